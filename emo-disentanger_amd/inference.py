"""Autoregressive generation — the sampling loop of
/root/reference/stage2_accompaniment/inference.py (temperature :71-83, nucleus :86-100,
generate_conditional :231-327) on top of a recurrent-state / KV-cache decode engine.

The reference re-runs the full model over the whole (<=2048-token) prefix for every sampled token
(SURVEY F7).  Here the Performer keeps its FAVOR+ scan state (S [F x dh], z [F] per layer/head) and
GPT-2 keeps a KV cache in HBM, so a step costs one token of work; results equal full recompute
(tests/test_gpu_generate.py).  Rejected samples (Beat going backwards, PAD, early EOS) re-sample from
the SAME logits without touching the state.  Once the window slides (len >= 2048) absolute positions
restart at 0 every step, which invalidates any cache: the engine then falls back to the reference's
full-window forward.  Host-side sampling helpers keep the reference's NumPy semantics (global RNG,
F12 nucleus indexing); `sample_on_device` is the batched on-GPU path (emo_sample_nucleus).
"""
import os
import time

import numpy as np
import torch

from . import engine, ops, scoring
from ._lib import EmoError
from .gen_loop import GrammarLoop, check_vocab, draw_controls
from .replay import StepReplayer, graph_steps

max_dec_inp_len = 2048


# ------------------------------------------------------------------------------------------------ sampling
from .sampling import beat_position, event_name, nucleus, temperature  # noqa: E402,F401  (host path with the reference's NumPy semantics)


def uniform_table(rows, n, seed, device):
    """fp32 [rows, n] uniforms of a device generator seeded with `seed`: the draws of the device loops (row = draw number, column = stream)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    return torch.rand(rows, n, device=device, generator=gen)


def sample_on_device(logits, temp, top_p, u=None, greedy=False):
    """logits fp32 [n, V] on the GPU -> int64 [n] (no host round trip)."""
    if greedy:
        return ops.argmax(logits.contiguous())
    if u is None:
        u = torch.rand(logits.shape[0], device=logits.device)
    return ops.sample_nucleus(logits.contiguous(), temp, top_p, u)


# ------------------------------------------------------------------------------------------------ decode engines
class _EngineBase:
    def __init__(self, model, n_streams, max_len=max_dec_inp_len):
        self.model, self.n, self.max_len = model, n_streams, max_len
        self.ps = model._ensure_store()
        self.dev, self.dt = self.ps.device, self.ps.compute_dtype
        self.pos = 0
        self.pos_dev = torch.zeros(n_streams, device=self.dev, dtype=torch.int64)   # device-side positions (hipGraph replay)
        self._tables = None
        self.dev_pos0, self.pos_auto = 0, True   # position = dev_pos0 + pos_dev[stream]; pos_auto: the engine advances pos_dev itself

    def _inputs(self):
        """-> (token table, segment table or None, positional table): the embedding tables are a snapshot, like the engine's omegas / folded weights."""
        m = self.model
        if self._tables is None:
            self._tables = (engine.embedding_table(self.ps, 'token_emb.'), engine.embedding_table(self.ps, 'segemb.') if m.use_segment_emb else None)
        return self._tables + (m.pe.pe if m.use_pe else m._zero_pe(self.max_len, m.d_model),)

    def _embed(self, tok, seg, pos0, dev_pos=False):
        m = self.model
        E, S, pe = self._inputs()
        S = S if seg is not None else None
        return ops.embed_fwd(tok, seg if S is not None else None, E, S, pe, self.dt, float(m.token_emb.emb_scale),
                             pos0=self.dev_pos0 if dev_pos else pos0, pos_ids=self.pos_dev if dev_pos else None).view(-1, m.d_model)

    def _advance(self, dev_pos):
        """One position further: the host count, or the device array unless the caller's own kernel advances it (pos_auto False)."""
        if not dev_pos:
            self.pos += 1
        elif self.pos_auto:
            self.pos_dev.add_(1)

    def _logits(self, h, out=None):
        return ops.gemm(h, self.ps.w('dec_out_proj.weight'), bias=self.ps.f32('dec_out_proj.bias'), out=out, out_dtype=torch.float32)

    def _check_lens(self, tok, lens):
        """The per-row lengths of prefill(lens=): int32 [B] on the engine's device."""
        if lens.dtype != torch.int32 or lens.shape != (tok.shape[0],) or lens.device != tok.device:
            raise EmoError('prefill(lens=): lens must be int32 [%d] on the device of the tokens' % tok.shape[0])
        return lens.contiguous()

    def _rows_at(self, x, lens, B, T):
        """Rows lens[b] - 1 of the hidden states x [B*T, D], and the engine's positions set to the rows' own: pos_dev = lens (in place: the
        array's address may sit in an argument block), dev_pos0 = 0, the host count at the longest row."""
        at = torch.arange(B, device=self.dev) * T + (lens.long() - 1).clamp_(0, T - 1)
        self.pos = T
        self.pos_dev.copy_(lens)
        self.dev_pos0 = 0
        return x.index_select(0, at).contiguous()

    @torch.no_grad()
    def append(self, tok, seg):
        """tok, seg: int64 [n, k]; consumes k tokens per stream, returns logits [n, V] after the last one."""
        if self.pos == 0:
            return self.prefill(tok, seg)
        out = None
        for i in range(tok.shape[1]):
            out = self.step(tok[:, i], seg[:, i])
        return out

    # ------------------------------------------------------------------------------------------ one-launch step (what the two engines share)
    # An engine with one supplies: step_entry (the form's name in emo_decode_step's messages), _persist_layer(l, t_qkv, t_one, t_ffn) -> the 12
    # weight tensors of layer l, _persist_state(l) -> its last four table columns, _check_position(pe) and _persist_form() -> the fields of the
    # argument block that are the form's own.  The base class owns the block (persist['args'], one per engine) and both launches.
    _pos_field = 'pos_ids'                                           # the field that takes the device positions of a step
    _TABLE_COLS = ('wqkv', 'bqkv', 'wo', 'bo', 'g1', 'be1', 'w1', 'b1', 'w2', 'b2', 'g2', 'be2')

    @staticmethod
    def _pack_fragments(W, tile_idx, kpw):
        """bf16 nn.Linear weight [N, K] -> [members][4 waves][tiles per member][kpw][64 lanes x 8]: the MFMA B fragment (16 output columns x 32 k)
        of column tile t and k step ks holds, in lane l, W[16 t + l % 16][32 ks + 8 (l // 16) .. + 8]; wave w of the compute half that owns the
        product holds the k steps [w kpw, (w + 1) kpw) of all of the member's tiles (emo_hip.h: emo_decode_step_t.layer_table)."""
        N, K = W.shape
        assert N % 16 == 0 and K == 32 * 4 * kpw
        frags = W.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(N // 16, K // 32, 512)      # [tile][k step][lane * 8 + j]
        sel = frags[tile_idx]                                                                                  # [members, tiles per member, k steps, 512]
        members, tpm = tile_idx.shape
        return sel.reshape(members, tpm, 4, kpw, 512).permute(0, 2, 1, 3, 4).contiguous()

    def _prepare_persist(self):
        m, ps, dev = self.model, self.ps, self.dev
        mem = torch.arange(32, device=dev)
        t_qkv = torch.stack([mem, 32 + mem, 64 + mem], 1)            # member (h, j) = 4 h + j: rows 64 h + 16 j .. of q, of k (+ 512), of v (+ 1024)
        t_one = mem.view(32, 1)                                      # member m: output columns 16 m ..
        t_ffn = (4 * mem).view(32, 1) + torch.arange(4, device=dev).view(1, 4)
        self.persist = {'w': [self._persist_layer(l, t_qkv, t_one, t_ffn) for l in range(m.n_layer)], 'table': None}
        V = m.n_token
        Vp = (V + 15) // 16 * 16
        wout = torch.zeros(Vp, m.d_model, device=dev, dtype=torch.bfloat16)
        wout[:V] = ps.w('dec_out_proj.weight')
        self.persist['wout'] = self._pack_fragments(wout, torch.arange(Vp // 16, device=dev).view(-1, 1), 4)
        self.persist['bout'] = ps.f32('dec_out_proj.bias')
        self.persist['sync'] = torch.zeros(ops.lib.emo_decode_step_workspace_bytes() // 8, device=dev, dtype=torch.int64)   # zeroed ONCE
        self.persist['logits'] = torch.zeros(self.n_pad, V, device=dev, dtype=torch.float32)
        if self.n_pad != self.n:                                     # padded inputs of the idle streams: token 0, segment 0, position 0
            self.persist['tok'] = torch.zeros(self.n_pad, dtype=torch.int64, device=dev)
            self.persist['seg'] = torch.zeros(self.n_pad, dtype=torch.int64, device=dev)
            self.persist['pos'] = torch.zeros(self.n_pad, dtype=torch.int64, device=dev)
        # the argument block of the launch (emo_hip.h: emo_decode_step_t): what never changes is written here, once; persist['held'] keeps the
        # tensors behind its addresses alive.  A step writes only its inputs, its output and — sampled — the sampler's fields.
        E, Sg, pe = self._inputs()
        pp = self.persist
        pp['args'], pp['held'], pp['pe'] = ops.DecodeStep(), {}, pe
        ops.decode_step_set(pp['args'], pp['held'], n_layers=m.n_layer, E=E, Sg=Sg, pe=pe, wout_packed=pp['wout'], bout=pp['bout'], n_token=V,
                            n_streams=self.n_pad, n_real=self.n, d_model=m.d_model, n_head=m.n_head, d_ff=2048, sync_ws=pp['sync'], ln_eps=1e-5,
                            **self._persist_form())

    def _void_table(self):
        """New state tensors (a prefill): the pointer table is rebuilt at the next step, and the block must not keep the address of the old one."""
        self.persist['table'] = None
        ops.decode_step_set(self.persist['args'], self.persist['held'], layer_table=None)

    def _launch(self, sampled, **fields):
        """The one-launch step on the engine's argument block.  The [L][16] pointer table (emo_hip.h) is built at the first step after the state
        tensors exist."""
        pp = self.persist
        if pp['table'] is None:
            rows = [[w[c].data_ptr() for c in self._TABLE_COLS] + self._persist_state(l) for l, w in enumerate(pp['w'])]
            pp['table'] = torch.tensor(rows, dtype=torch.int64, device=self.dev)
            fields['layer_table'] = pp['table']
        ops.decode_step_set(pp['args'], pp['held'], sampled=sampled, **fields)
        ops.decode_step(pp['args'])

    def _step_persistent(self, tok, seg, dev_pos, logits_out):
        """Returns `logits_out` when given, else the engine's STATIC logits buffer (or a view of its first n rows): the next step overwrites it —
        callers that keep logits across steps clone them (the chain of launches returns a fresh tensor; hipGraph capture needs the static one)."""
        pp = self.persist
        seg = seg if (pp['held']['Sg'] is not None and seg is not None) else None
        if not dev_pos:
            self._check_position(pp['pe'])                           # (ops.embed_fwd makes the same check on the launch-chain path)
        pos_ids = self.pos_dev if dev_pos else None
        padded = self.n_pad != self.n
        if padded:
            pp['tok'][:self.n].copy_(tok)
            tok = pp['tok']
            if seg is not None:
                pp['seg'][:self.n].copy_(seg)
                seg = pp['seg']
            if pos_ids is not None:
                pp['pos'][:self.n].copy_(pos_ids)
                pos_ids = pp['pos']
        out = logits_out if (logits_out is not None and not padded) else pp['logits']
        self._launch(0, tok=tok, seg=seg, pos0=self.dev_pos0 if dev_pos else self.pos, logits=out, diag=pp.get('diag'), **{self._pos_field: pos_ids})
        if padded:
            if logits_out is not None:
                logits_out.copy_(out[:self.n])
                return logits_out
            return out[:self.n]
        return out

    def step_sampled(self, seg_padded, temp, top_p, U, step_ctr, seq, col0, tok_out, pos0):
        """One token step with the nucleus draw INSIDE the launch (emo_decode_step_t.sampled): draws from the logits the previous step (or the
        prefill: see load_logits) left in the engine's buffer, writes token / sequence / step counter like emo_sample_nucleus_step, then runs
        the step on the drawn tokens.  seg_padded: int64 [n_pad] (or None)."""
        pp = self.persist
        self._launch(1, seg=seg_padded if pp['held']['Sg'] is not None else None, pos0=pos0, logits=pp['logits'], diag=None, temperature=temp, top_p=top_p,
                     u_steps=U, step=step_ctr, seq=seq, col0=col0, tok_out=tok_out)
        return pp['logits'][:self.n]

    def load_logits(self, logits):
        """Put externally produced logits (the prefill's) where step_sampled draws from."""
        self.persist['logits'][:self.n].copy_(logits)

    def check_persistent(self):
        """Raises if a one-launch step gave up (synchronises; call it where the caller reads results anyway)."""
        if self.persist is not None:
            code = int(self.persist['sync'][-8].item())
            if code != 0:
                raise EmoError('%s gave up (code 0x%x): a workgroup of the persistent launch did not get a compute unit next to the others within '
                               '50 ms (is another process using the GPU?); set EMO_DECODE_PERSISTENT=0 for the chain of launches' % (self.step_entry, code))


class PerformerDecodeEngine(_EngineBase):
    """FAVOR+ recurrent state per layer: S [n,H,F,dh], z [n,H,F] fp32 (6.4 MB / stream at the perf config).
    omega is fixed for the lifetime of the engine (the state is only meaningful under one feature map)."""

    def __init__(self, model, n_streams, redraw=True, persistent=True):
        """persistent=False keeps the chain of launches (callers that run several engines side by side on different streams, and the fall-back of
        the reference loop when a one-launch step gave up)."""
        super().__init__(model, n_streams)
        if redraw and model.redraw != 'fixed':
            model.draw_feature_maps()
        self.omegas = [lyr.attention.inner_attention.feature_map.omega.clone() for lyr in model.transformer_decoder.decoder_layers]
        self.act = ops.ACT_GELU if getattr(model, 'activation', 'relu') == 'gelu' else ops.ACT_RELU
        self.S, self.z = [None] * model.n_layer, [None] * model.n_layer
        # bf16 one-token steps: norm1 / norm2 are folded into the GEMMs around them (2 launches fewer per layer, see emo_hip.h: ln_c1 / rln_*)
        self.fold = None
        if self.dt == torch.bfloat16 and n_streams <= 32 and os.environ.get('EMO_DECODE_LN_FOLD', '1') != '0':
            self._prepare_folds()
        # the whole token step as ONE persistent launch (emo_decode_step, form 0) for the benchmark architecture: bf16, d_model 512, 8 heads,
        # 128 features, d_ff 2048, up to 32 streams (the kernel's groups own 4 streams each: other counts — the reference's own one-piece-at-a-time
        # loop is n = 1 — are padded with idle streams whose state is zero and whose logits nobody reads).  EMO_DECODE_PERSISTENT=0 keeps the chain
        # of launches (tests compare the two).
        self.persist = None
        ff = model.transformer_decoder.decoder_layers[0].linear1.weight.shape[0]
        nf = 2 * self.omegas[0].shape[1]
        self.n_pad = (n_streams + 3) // 4 * 4
        if (self.dt == torch.bfloat16 and 1 <= n_streams <= 32 and model.d_model == 512 and model.n_head == 8 and nf == 128
                and ff == 2048 and model.n_layer <= 15 and model.n_token <= 512 and persistent and self.act == ops.ACT_RELU
                and os.environ.get('EMO_DECODE_PERSISTENT', '1') != '0'
                and ops.lib.emo_decode_step_supported() == 1):
            # (emo_decode_step_supported: the launch's 256 workgroups spin-wait on each other and must all be resident — >= 256 CUs,
            # 96 KB LDS each, one per CU by the occupancy query; partitions / CU masks with fewer keep the chain of launches)
            self._prepare_persist()

    def start_empty(self):
        """Every row at S = 0, z = 0, as before its first token: the start of a loop without a prefill (AccompanimentQueue), whose rows are
        restarted one by one later on (ops.favor_state_reset).  -> the int64 [n_layer, 2] device table of the S / z base addresses."""
        m = self.model
        H, F = m.n_head, 2 * self.omegas[0].shape[1]
        rows = self.n_pad if self.persist is not None else self.n        # (the idle padding rows of the one-launch step: zero like the others)
        for l in range(m.n_layer):
            self.S[l] = torch.zeros(rows, H, F, m.d_model // H, device=self.dev, dtype=torch.float32)[:self.n]
            self.z[l] = torch.zeros(rows, H, F, device=self.dev, dtype=torch.float32)[:self.n]
        if self.persist is not None:
            self._void_table()
        return torch.tensor([[self.S[l].data_ptr(), self.z[l].data_ptr()] for l in range(m.n_layer)], dtype=torch.int64, device=self.dev)

    # ------------------------------------------------------------------------------------------ one-launch step
    step_entry = 'emo_decode_step[performer]'

    def _persist_layer(self, l, t_qkv, t_one, t_ffn):
        m, ps, pk = self.model, self.ps, self._pack_fragments
        D = m.d_model
        pfx = m._layer_prefix(l)
        q = pfx + 'attention.query_projection.'
        return dict(wqkv=pk(ps.w(q + 'weight', 3 * D), t_qkv, 4), bqkv=ps.f32(q + 'bias', 3 * D),
                    wo=pk(ps.w(pfx + 'attention.out_projection.weight'), t_one, 4), bo=ps.f32(pfx + 'attention.out_projection.bias'),
                    g1=ps.f32(pfx + 'norm1.weight'), be1=ps.f32(pfx + 'norm1.bias'),
                    w1=pk(ps.w(pfx + 'linear1.weight'), t_ffn, 4), b1=ps.f32(pfx + 'linear1.bias'),
                    w2=pk(ps.w(pfx + 'linear2.weight'), t_one, 16), b2=ps.f32(pfx + 'linear2.bias'),
                    g2=ps.f32(pfx + 'norm2.weight'), be2=ps.f32(pfx + 'norm2.bias'))

    def _persist_state(self, l):
        assert self.S[l].is_contiguous() and self.z[l].is_contiguous() and self.omegas[l].is_contiguous()
        return [self.omegas[l].data_ptr(), self.S[l].data_ptr(), self.z[l].data_ptr(), 0]

    def _check_position(self, pe):
        if self.pos >= pe.shape[0]:
            raise EmoError('decode position %d is past the positional-encoding table (%d rows)' % (self.pos, pe.shape[0]))

    def _persist_form(self):
        return dict(form=0, emb_scale=float(self.model.token_emb.emb_scale), n_feat=2 * self.omegas[0].shape[1], eps=1e-6)

    def _prepare_folds(self):
        """gamma-scaled weights, c1[n] = sum_k gamma_k W[n,k] (of the ROUNDED bf16 product, the one the MFMA sees) and bias + W.beta for every
        GEMM whose input is a LayerNorm output: linear1 (norm1), the next layer's q/k/v projection and the final logits (norm2).  Built once
        per engine from the fp32 masters: the engine is a snapshot of the weights, like its omegas."""
        m, ps = self.model, self.ps
        D = m.d_model

        def fold(wname, bname, rows, gamma, beta):
            W = ps.f32(wname, rows)
            Wg = (W * gamma[None, :]).to(torch.bfloat16).contiguous()
            return Wg, Wg.float().sum(1).contiguous(), (ps.f32(bname, rows) + (W * beta[None, :]).sum(1)).contiguous()

        L = m.n_layer
        pf = [m._layer_prefix(l) for l in range(L)]
        self.fold = {'ffn1': [fold(pf[l] + 'linear1.weight', pf[l] + 'linear1.bias', None, ps.f32(pf[l] + 'norm1.weight'), ps.f32(pf[l] + 'norm1.bias'))
                              for l in range(L)],
                     'qkv': [None] + [fold(pf[l] + 'attention.query_projection.weight', pf[l] + 'attention.query_projection.bias', 3 * D,
                                           ps.f32(pf[l - 1] + 'norm2.weight'), ps.f32(pf[l - 1] + 'norm2.bias')) for l in range(1, L)],
                     'out': fold('dec_out_proj.weight', 'dec_out_proj.bias', None, ps.f32(pf[L - 1] + 'norm2.weight'), ps.f32(pf[L - 1] + 'norm2.bias'))}
        self.stats1 = torch.empty(self.n, 2, device=self.dev, dtype=torch.float32)
        self.stats2 = torch.empty(self.n, 2, device=self.dev, dtype=torch.float32)

    def _step_folded(self, x, logits_out):
        """One token per stream, LayerNorms folded: per layer q/k/v GEMM, state update, out-projection, linear1, linear2 (5 launches)."""
        m, ps, fd = self.model, self.ps, self.fold
        D, H = m.d_model, m.n_head
        res = None                                   # (raw tensor, stats, gamma, beta) whose LayerNorm is the current hidden state
        for l in range(m.n_layer):
            pfx = m._layer_prefix(l)
            q = pfx + 'attention.query_projection.'
            if res is None:
                qkv = ops.gemm(x, ps.w(q + 'weight', 3 * D), bias=ps.f32(q + 'bias', 3 * D))
            else:
                Wg, c1, bb = fd['qkv'][l]
                qkv = ops.gemm(res[0], Wg, bias=bb, ln_c1=c1, ln_stats_out=self.stats2)
            attn = ops.favor_decode_step(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], self.omegas[l], self.S[l], self.z[l], H)
            ow, ob = ps.w(pfx + 'attention.out_projection.weight'), ps.f32(pfx + 'attention.out_projection.bias')
            x1 = ops.gemm(attn, ow, bias=ob, residual=x) if res is None else ops.gemm(attn, ow, bias=ob, rln=res)
            Wg, c1, bb = fd['ffn1'][l]
            f = ops.gemm(x1, Wg, bias=bb, act=self.act, ln_c1=c1, ln_stats_out=self.stats1)
            x2 = ops.gemm(f, ps.w(pfx + 'linear2.weight'), bias=ps.f32(pfx + 'linear2.bias'),
                          rln=(x1, self.stats1, ps.f32(pfx + 'norm1.weight'), ps.f32(pfx + 'norm1.bias')))
            res = (x2, self.stats2, ps.f32(pfx + 'norm2.weight'), ps.f32(pfx + 'norm2.bias'))
        Wg, c1, bb = fd['out']
        return ops.gemm(res[0], Wg, bias=bb, ln_c1=c1, out=logits_out, out_dtype=torch.float32)

    @torch.no_grad()
    def prefill(self, tok, seg, lens=None):
        """lens (int32 [B] on the device, 1 <= lens[b] <= T): row b holds lens[b] tokens and padding behind them.  Causality keeps the attention
        outputs below lens[b] independent of the padding; the state is the row's own (ops.favor_state_at, not the scan's end state), the logits
        returned are those of position lens[b] - 1 and every row steps on from its own position (pos_dev = lens, dev_pos0 = 0)."""
        if lens is not None:
            return self._prefill_varlen(tok, seg, self._check_lens(tok, lens))
        m, ps = self.model, self.ps
        B, T = tok.shape
        D, H = m.d_model, m.n_head
        x = self._embed(tok, seg, 0)
        for l in range(m.n_layer):
            pfx = m._layer_prefix(l)
            q = pfx + 'attention.query_projection.'
            qkv = ops.gemm(x, ps.w(q + 'weight', 3 * D), bias=ps.f32(q + 'bias', 3 * D))
            attn, _, self.S[l], self.z[l] = ops.favor_attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], self.omegas[l], B, T, H, want_state=True)
            x = self._tail(pfx, x, attn)
        if self.persist is not None:
            self._void_table()
            if self.n_pad != B:                                  # state of the padded (idle) streams: zero; S[l] / z[l] stay the views of the real ones
                for l in range(m.n_layer):
                    Sp = torch.zeros((self.n_pad,) + tuple(self.S[l].shape[1:]), device=self.dev, dtype=self.S[l].dtype)
                    zp = torch.zeros((self.n_pad,) + tuple(self.z[l].shape[1:]), device=self.dev, dtype=self.z[l].dtype)
                    Sp[:B].copy_(self.S[l])
                    zp[:B].copy_(self.z[l])
                    self.S[l], self.z[l] = Sp[:B], zp[:B]
        self.pos = T
        self.pos_dev.fill_(T)
        return self._logits(x.view(B, T, D)[:, -1].contiguous())

    def _prefill_varlen(self, tok, seg, lens):
        m, ps = self.model, self.ps
        B, T = tok.shape
        D, H = m.d_model, m.n_head
        F = 2 * self.omegas[0].shape[1]
        rows = self.n_pad if self.persist is not None else B     # (the idle padding rows of the one-launch step: zero, as in prefill)
        x = self._embed(tok, seg, 0)
        for l in range(m.n_layer):
            pfx = m._layer_prefix(l)
            q = pfx + 'attention.query_projection.'
            qkv = ops.gemm(x, ps.w(q + 'weight', 3 * D), bias=ps.f32(q + 'bias', 3 * D))
            attn, _ = ops.favor_attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], self.omegas[l], B, T, H)
            Sp = torch.zeros(rows, H, F, D // H, device=self.dev, dtype=torch.float32)
            zp = torch.zeros(rows, H, F, device=self.dev, dtype=torch.float32)
            self.S[l], self.z[l] = Sp[:B], zp[:B]
            ops.favor_state_at(qkv[:, D:2 * D], qkv[:, 2 * D:], self.omegas[l], lens, B, T, H, out=(self.S[l], self.z[l]))
            x = self._tail(pfx, x, attn)
        if self.persist is not None:
            self._void_table()
        return self._logits(self._rows_at(x, lens, B, T))

    def _tail(self, pfx, x, attn):
        ps = self.ps
        x1 = ops.gemm(attn, ps.w(pfx + 'attention.out_projection.weight'), bias=ps.f32(pfx + 'attention.out_projection.bias'), residual=x)
        h1, _, _ = ops.layernorm_fwd(x1, ps.f32(pfx + 'norm1.weight'), ps.f32(pfx + 'norm1.bias'))
        f = ops.gemm(h1, ps.w(pfx + 'linear1.weight'), bias=ps.f32(pfx + 'linear1.bias'), act=self.act)
        x2 = ops.gemm(f, ps.w(pfx + 'linear2.weight'), bias=ps.f32(pfx + 'linear2.bias'), residual=h1)
        out, _, _ = ops.layernorm_fwd(x2, ps.f32(pfx + 'norm2.weight'), ps.f32(pfx + 'norm2.bias'))
        return out

    @torch.no_grad()
    def step(self, tok, seg, dev_pos=False, logits_out=None):
        """dev_pos=True: positions come from the device array `pos_dev` (and are advanced on the device), so the whole step is
        capturable in a hipGraph and replayable.  logits_out: write the logits into this static buffer (no copy kernel)."""
        m, ps = self.model, self.ps
        D, H = m.d_model, m.n_head
        if self.persist is not None:
            out = self._step_persistent(tok.reshape(-1), None if seg is None else seg.reshape(-1), dev_pos, logits_out)
            self._advance(dev_pos)
            return out
        x = self._embed(tok.view(-1, 1), None if seg is None else seg.view(-1, 1), self.pos, dev_pos)
        if self.fold is not None:
            out = self._step_folded(x, logits_out)
            self._advance(dev_pos)
            return out
        for l in range(m.n_layer):
            pfx = m._layer_prefix(l)
            q = pfx + 'attention.query_projection.'
            qkv = ops.gemm(x, ps.w(q + 'weight', 3 * D), bias=ps.f32(q + 'bias', 3 * D))
            attn = ops.favor_decode_step(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], self.omegas[l], self.S[l], self.z[l], H)
            x = self._tail(pfx, x, attn)
        self._advance(dev_pos)
        return self._logits(x, logits_out)


class GPT2DecodeEngine(_EngineBase):
    """KV cache in HBM: per layer k,v [n, max_len, D] in the compute dtype (1.6 GB for 32 streams x 2048 x 12 layers, bf16)."""

    def __init__(self, model, n_streams, max_len=max_dec_inp_len, persistent=True):
        super().__init__(model, n_streams, max_len)
        D = model.d_model
        self.n_pad = (n_streams + 3) // 4 * 4
        # head-major cache [n, H, max_len, dh] (r06; HF's own past_key_values layout): the decode attention gives one workgroup to a (stream, head),
        # whose keys are then one contiguous run instead of 128-byte pieces 1 KB apart.  EMO_KV_HEAD_MAJOR=0: [n, max_len, D] (r05, same-box A/B)
        self.head_major = os.environ.get('EMO_KV_HEAD_MAJOR', '1') != '0'
        # the whole token step as ONE persistent launch (emo_decode_step, form 1; r06), under the conditions of the Performer engine's: bf16, d_model 512,
        # 8 heads, d_ff 2048, <= 32 streams (padded to a multiple of 4 with idle streams), head-major cache of <= 2048 rows.  EMO_DECODE_PERSISTENT=0 /
        # EMO_GPT2_PERSISTENT=0 keep the chain of launches (tests compare the two).
        ff = self.ps.f32(model._layer_prefix(0) + 'mlp.c_fc.bias').numel()
        want_persist = (self.dt == torch.bfloat16 and 1 <= n_streams <= 32 and D == 512 and model.n_head == 8 and ff == 2048 and model.n_layer <= 15
                        and model.n_token <= 512 and max_len <= 2048 and self.head_major and persistent
                        and os.environ.get('EMO_DECODE_PERSISTENT', '1') != '0' and os.environ.get('EMO_GPT2_PERSISTENT', '1') != '0'
                        and ops.lib.emo_decode_step_supported() == 1)
        rows = self.n_pad if want_persist else n_streams
        shp = (rows, model.n_head, max_len, D // model.n_head) if self.head_major else (rows, max_len, D)
        self.kc_all = [torch.zeros(*shp, device=self.dev, dtype=self.dt) for _ in range(model.n_layer)]
        self.vc_all = [torch.zeros(*shp, device=self.dev, dtype=self.dt) for _ in range(model.n_layer)]
        self.kc = [t[:n_streams] for t in self.kc_all]             # (rows n .. n_pad: the idle padding streams of the one-launch step)
        self.vc = [t[:n_streams] for t in self.vc_all]
        self.persist = None
        self.lens = torch.zeros(n_streams, device=self.dev, dtype=torch.int64)
        # bf16 one-token steps: the Conv1D weights ([in, out]) are transposed ONCE to the k-contiguous layout of the skinny decode GEMM,
        # ln_1 / ln_2 are folded into c_attn / c_fc (emo_hip.h: ln_c1) and the new k / v rows are appended by the attention kernel:
        # 5 launches per layer instead of 9 general-shape ones.
        self.fold = None
        if self.dt == torch.bfloat16 and n_streams <= 32 and os.environ.get('EMO_DECODE_LN_FOLD', '1') != '0':
            self._prepare_folds()
        if want_persist:
            self._prepare_persist()

    # ------------------------------------------------------------------------------------------ one-launch step
    step_entry = 'emo_decode_step[gpt2]'

    def _persist_form(self):
        ps, p0 = self.ps, self.model._layer_prefix(0)
        return dict(form=1, emb_scale=float(self.model.token_emb.emb_scale), kv_tmax=self.max_len,
                    ln0=torch.cat([ps.f32(p0 + 'ln_1.weight'), ps.f32(p0 + 'ln_1.bias')]).contiguous())

    def _persist_layer(self, l, t_qkv, t_one, t_ffn):
        m, ps, pk = self.model, self.ps, self._pack_fragments

        def lin(name):                                               # Conv1D [in, out] -> nn.Linear layout [out, in]
            return ps.w(name).t().contiguous()

        pfx = m._layer_prefix(l)
        nx = m._layer_prefix(l + 1 if l + 1 < m.n_layer else 0)      # (the last block's slot is loaded and never applied: this GPT-2 has no ln_f)
        return dict(wqkv=pk(lin(pfx + 'attn.c_attn.weight'), t_qkv, 4), bqkv=ps.f32(pfx + 'attn.c_attn.bias'),
                    wo=pk(lin(pfx + 'attn.c_proj.weight'), t_one, 4), bo=ps.f32(pfx + 'attn.c_proj.bias'),
                    g1=ps.f32(pfx + 'ln_2.weight'), be1=ps.f32(pfx + 'ln_2.bias'),
                    w1=pk(lin(pfx + 'mlp.c_fc.weight'), t_ffn, 4), b1=ps.f32(pfx + 'mlp.c_fc.bias'),
                    w2=pk(lin(pfx + 'mlp.c_proj.weight'), t_one, 16), b2=ps.f32(pfx + 'mlp.c_proj.bias'),
                    g2=ps.f32(nx + 'ln_1.weight'), be2=ps.f32(nx + 'ln_1.bias'))

    def _persist_state(self, l):
        return [0, self.kc_all[l].data_ptr(), self.vc_all[l].data_ptr(), 0]       # (the caches live as long as the engine)

    def _check_position(self, pe):
        rows = min(pe.shape[0], self.max_len)
        if self.pos >= rows:
            raise EmoError('decode position %d is past the positional-encoding table / the KV cache (%d rows)' % (self.pos, rows))

    def _prepare_folds(self):
        m, ps = self.model, self.ps

        def tr(wname, bname, gamma=None, beta=None):
            Wt = ps.f32(wname).t().contiguous()                    # [out, in]
            if gamma is None:
                return Wt.to(torch.bfloat16).contiguous(), None, ps.f32(bname)
            Wg = (Wt * gamma[None, :]).to(torch.bfloat16).contiguous()
            return Wg, Wg.float().sum(1).contiguous(), (ps.f32(bname) + (Wt * beta[None, :]).sum(1)).contiguous()

        self.fold = []
        for l in range(m.n_layer):
            pfx = m._layer_prefix(l)
            self.fold.append({'attn': tr(pfx + 'attn.c_attn.weight', pfx + 'attn.c_attn.bias', ps.f32(pfx + 'ln_1.weight'), ps.f32(pfx + 'ln_1.bias')),
                              'proj': tr(pfx + 'attn.c_proj.weight', pfx + 'attn.c_proj.bias'),
                              'fc': tr(pfx + 'mlp.c_fc.weight', pfx + 'mlp.c_fc.bias', ps.f32(pfx + 'ln_2.weight'), ps.f32(pfx + 'ln_2.bias')),
                              'mlp': tr(pfx + 'mlp.c_proj.weight', pfx + 'mlp.c_proj.bias')})

    def _step_folded(self, x, lens, lens_off, logits_out):
        m = self.model
        D, H = m.d_model, m.n_head
        for l in range(m.n_layer):
            fd = self.fold[l]
            Wg, c1, bb = fd['attn']
            qkv = ops.gemm(x, Wg, bias=bb, ln_c1=c1)
            a = ops.softmax_attn_decode(qkv[:, :D], self.kc[l], self.vc[l], lens, H, lens_off=lens_off, k_new=qkv[:, D:2 * D], v_new=qkv[:, 2 * D:])
            Wt, _, bb = fd['proj']
            h = ops.gemm(a, Wt, bias=bb, residual=x)
            Wg, c1, bb = fd['fc']
            f = ops.gemm(h, Wg, bias=bb, act=ops.ACT_GELU_NEW, ln_c1=c1)
            Wt, _, bb = fd['mlp']
            x = ops.gemm(f, Wt, bias=bb, residual=h)
        return self._logits(x, logits_out)

    def _block_tail(self, pfx, x, a):
        ps = self.ps
        h = ops.gemm(a, ps.w(pfx + 'attn.c_proj.weight'), b_trans=True, bias=ps.f32(pfx + 'attn.c_proj.bias'), residual=x)
        n2, _, _ = ops.layernorm_fwd(h, ps.f32(pfx + 'ln_2.weight'), ps.f32(pfx + 'ln_2.bias'))
        f = ops.gemm(n2, ps.w(pfx + 'mlp.c_fc.weight'), b_trans=True, bias=ps.f32(pfx + 'mlp.c_fc.bias'), act=ops.ACT_GELU_NEW)
        return ops.gemm(f, ps.w(pfx + 'mlp.c_proj.weight'), b_trans=True, bias=ps.f32(pfx + 'mlp.c_proj.bias'), residual=h)

    @torch.no_grad()
    def prefill(self, tok, seg, lens=None):
        """lens (int32 [B] on the device, 1 <= lens[b] <= T): row b holds lens[b] tokens and padding behind them.  The cache rows at and beyond
        lens[b] then hold the padding's keys; the decode step overwrites each of them before it reads it (it appends at row lens[b], then
        attends over lens[b] + 1 rows).  The logits returned are those of position lens[b] - 1; self.lens = pos_dev = lens, dev_pos0 = 0."""
        if lens is not None:
            lens = self._check_lens(tok, lens)
        m, ps = self.model, self.ps
        B, T = tok.shape
        D, H = m.d_model, m.n_head
        x = self._embed(tok, seg, 0)
        for l in range(m.n_layer):
            pfx = m._layer_prefix(l)
            n1, _, _ = ops.layernorm_fwd(x, ps.f32(pfx + 'ln_1.weight'), ps.f32(pfx + 'ln_1.bias'))
            qkv = ops.gemm(n1, ps.w(pfx + 'attn.c_attn.weight'), b_trans=True, bias=ps.f32(pfx + 'attn.c_attn.bias'))
            if self.head_major:
                self.kc[l][:, :, :T].copy_(qkv[:, D:2 * D].view(B, T, H, D // H).permute(0, 2, 1, 3))
                self.vc[l][:, :, :T].copy_(qkv[:, 2 * D:].view(B, T, H, D // H).permute(0, 2, 1, 3))
            else:
                self.kc[l][:, :T].copy_(qkv[:, D:2 * D].view(B, T, D))
                self.vc[l][:, :T].copy_(qkv[:, 2 * D:].view(B, T, D))
            a, _ = ops.softmax_attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, T, H)
            x = self._block_tail(pfx, x, a)
        if lens is not None:
            self.lens.copy_(lens)
            return self._logits(self._rows_at(x, lens, B, T))
        self.pos = T
        self.pos_dev.fill_(T)
        self.lens.fill_(T)
        return self._logits(x.view(B, T, D)[:, -1].contiguous())

    @torch.no_grad()
    def step(self, tok, seg, dev_pos=False, logits_out=None):
        m, ps = self.model, self.ps
        D, H = m.d_model, m.n_head
        if self.persist is not None:
            out = self._step_persistent(tok.reshape(-1), None if seg is None else seg.reshape(-1), dev_pos, logits_out)
            self.lens.add_(1)
            self._advance(dev_pos)
            return out
        x = self._embed(tok.view(-1, 1), None if seg is None else seg.view(-1, 1), self.pos, dev_pos)
        if self.fold is not None:
            if dev_pos and not self.pos_auto:            # positions AND key counts come from the sampler's step counter
                return self._step_folded(x, self.pos_dev, self.dev_pos0 + 1, logits_out)
            self.lens.add_(1)
            out = self._step_folded(x, self.lens, 0, logits_out)
            self._advance(dev_pos)
            return out
        self.lens.add_(1)
        ext = dev_pos and not self.pos_auto                       # positions AND key counts come from the sampler's step counter (as in the folded path)
        for l in range(m.n_layer):
            pfx = m._layer_prefix(l)
            n1, _, _ = ops.layernorm_fwd(x, ps.f32(pfx + 'ln_1.weight'), ps.f32(pfx + 'ln_1.bias'))
            qkv = ops.gemm(n1, ps.w(pfx + 'attn.c_attn.weight'), b_trans=True, bias=ps.f32(pfx + 'attn.c_attn.bias'))
            # (the general-shape path — fp32 parity mode, more than 32 streams — lets the attention kernel append the rows as the folded path does)
            a = ops.softmax_attn_decode(qkv[:, :D], self.kc[l], self.vc[l], self.pos_dev if ext else self.lens, H, lens_off=self.dev_pos0 + 1 if ext else 0,
                                        k_new=qkv[:, D:2 * D], v_new=qkv[:, 2 * D:])
            x = self._block_tail(pfx, x, a)
        self._advance(dev_pos)
        return self._logits(x, logits_out)


def make_engine(model, n_streams, **kw):
    return PerformerDecodeEngine(model, n_streams, **kw) if model.kind == 'performer' else GPT2DecodeEngine(model, n_streams, **kw)


# ------------------------------------------------------------------------------------------------ reference loop
def generate_conditional(model, event2idx, idx2event, lead_sheet_events, primer,
                         max_events=10000, skip_check=False, max_bars=None,
                         temp=1.2, top_p=0.9, inadmissibles=None,
                         model_type="performer", use_cache=True, sampler=None, verbose=False):
    """Arguments and return value of the reference's generate_conditional (inference.py:231-327): the accompaniment of every
    lead-sheet bar is sampled token by token until the model emits Track_LeadSheet, then the next bar's lead sheet is injected.
    The grammar (Beat positions never go back, PAD / premature EOS rejected, 256 consecutive rejections = stuck) lives in
    `_Stream.offer`; this function is the one-stream driver of it.  `sampler(probs)` defaults to nucleus(probs, top_p) on NumPy's
    global RNG, like the reference.  use_cache=False (or a context at the 2048-token window) runs the reference's full-window
    forward per sampled token."""
    note = print if verbose else (lambda *a, **k: None)
    draw = sampler if sampler is not None else (lambda probs: nucleus(probs, top_p))
    dev = next(model.parameters()).device
    s = _Stream(event2idx, lead_sheet_events, primer, max_bars)
    primed = len(s.generated)
    eng = make_engine(model, 1) if use_cache else None
    cached = None
    t0 = time.time()
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            while not s.done:
                if eng is not None and len(s.generated) < max_dec_inp_len:
                    if s.consumed < len(s.generated):            # new tokens since the last step (a sampled word, or an injected bar)
                        cached = eng.append(torch.tensor([s.generated[s.consumed:]], dtype=torch.long, device=dev),
                                            torch.tensor([s.seg[s.consumed:]], dtype=torch.long, device=dev))
                        s.consumed = len(s.generated)
                    logits = cached                              # a rejected sample is re-drawn from the same logits
                else:
                    kw = {'attn_kwargs': {'omit_feature_map_draw': len(s.generated) > primed}} if model_type == 'performer' else {}
                    logits = model(torch.tensor([s.generated[-max_dec_inp_len:]], dtype=torch.long, device=dev),
                                   seg_inp=torch.tensor([s.seg[-max_dec_inp_len:]], dtype=torch.long, device=dev), keep_last_only=True, **kw)
                logits_np = logits[0].cpu().numpy().copy()
                if eng is not None and getattr(eng, 'persist', None) is not None:
                    try:
                        eng.check_persistent()                   # (the copy above already synchronised)
                    except EmoError as e:
                        # the one-launch step gave up (its workgroups were not all resident within 50 ms): logits and recurrent state of this
                        # engine are void.  Re-run the piece so far through the chain of launches and continue there.
                        note('[gen] %s -> falling back to the chain of launches' % e)
                        eng = make_engine(model, 1, redraw=False, persistent=False) if model.kind == 'performer' else make_engine(model, 1, persistent=False)
                        s.consumed, cached = 0, None
                        continue
                probs = temperature(logits_np, temp, inadmissibles=inadmissibles)
                bars = s.generated_bars
                if not s.offer(int(draw(probs)), event2idx, idx2event, skip_check, max_events):
                    note('[gen] sample rejected (%d in a row)' % s.failed_cnt)
                elif s.generated_bars != bars:
                    note('[gen] bar %d / %d done, %d events' % (s.generated_bars, s.target_bars, len(s.generated)))
    finally:
        model.train(was_training)
    note('[gen] %d events in %.2f s%s' % (len(s.generated), time.time() - t0, ' (stuck: 256 rejected samples)' if s.stuck else ''))
    return s.result()


# ------------------------------------------------------------------------------------------------ batched reference loop (SURVEY f-4)
class _Stream:
    """Per-stream state of generate_conditional's loop (inference.py:233-250)."""

    def __init__(self, event2idx, lead_sheet_events, primer, max_bars):
        self.lead = lead_sheet_events
        self.generated = list(primer) + [event2idx['Track_LeadSheet']] + list(lead_sheet_events[0]) + [event2idx['Track_Full']]
        self.seg = [0] * len(self.generated)
        self.seg[-1] = 1
        self.target_bars = len(lead_sheet_events) if max_bars is None else min(max_bars, len(lead_sheet_events))
        self.generated_bars, self.cur_pos, self.failed_cnt = 0, 0, 0
        self.consumed = 0            # tokens already folded into the engine state
        self.done, self.stuck = self.target_bars <= 0, False

    def offer(self, word, event2idx, idx2event, skip_check, max_events):
        """One sampled word through the grammar of inference.py:276-318.  Returns False when the sample is rejected (the caller
        re-samples from the SAME distribution, like the reference's `continue`), True when the stream advanced or ended."""
        ev = idx2event[word]
        if not skip_check and 'Beat' in ev:
            pos = beat_position(ev)
            if not pos >= self.cur_pos:
                self.failed_cnt += 1
                if self.failed_cnt >= 256:          # reference: returns `generated` as is (no [:-1])
                    self.done = self.stuck = True
                    return True
                return False
            self.cur_pos, self.failed_cnt = pos, 0
        if ev == 'Track_LeadSheet':
            self.generated.append(word)
            self.seg.append(0)
            self.generated_bars += 1
            if self.generated_bars < self.target_bars:
                nxt = self.lead[self.generated_bars]
                self.generated.extend(nxt)
                self.seg.extend([0] * len(nxt))
                self.generated.append(event2idx['Track_Full'])
                self.seg.append(1)
                self.cur_pos = 0
            else:
                self.done = True
            return True
        if ev == 'PAD_None' or (ev == 'EOS_None' and self.generated_bars < self.target_bars - 1):
            return False
        if ev == 'EOS_None' and self.generated_bars == self.target_bars - 1:
            self.generated.append(word)
            self.done = True
            return True
        self.generated.append(word)
        self.seg.append(1)
        if len(self.generated) > max_events:
            self.done = True
        return True

    def result(self):
        return self.generated if self.stuck else self.generated[:-1]


def generate_conditional_batch(model, event2idx, idx2event, lead_sheets, primers, max_events=10000, skip_check=False, max_bars=None,
                               temp=1.2, top_p=0.9, inadmissibles=None, samplers=None, seeds=None):
    """n independent generate_conditional() runs (one lead sheet + primer each) in lock-step on ONE decode engine: per-stream bar
    counter, Beat position, rejection counter and RNG; every engine step feeds each unfinished stream its next pending token (a
    sampled word, or the next token of an injected lead-sheet bar), so streams of different lengths stay aligned in position.
    `samplers[i](probs)` defaults to nucleus(probs, top_p, rng=RandomState(seeds[i])).  Stream i returns exactly what
    generate_conditional(..., sampler=samplers[i]) returns for it alone (tests/test_gpu_generate.py), as long as it stays inside
    the 2048-token window (max_dec_inp_len); a stream that reaches the window is finished by the single-stream windowed path."""
    n = len(lead_sheets)
    assert n == len(primers) and n > 0
    if samplers is None:
        rss = [np.random.RandomState((seeds[i] if seeds is not None else i)) for i in range(n)]
        samplers = [(lambda probs, rs=rs: nucleus(probs, top_p, rng=rs)) for rs in rss]
    dev = next(model.parameters()).device
    st = [_Stream(event2idx, lead_sheets[i], primers[i], max_bars) for i in range(n)]
    pad = event2idx.get('PAD_None', 0)
    was_training = model.training
    model.eval()
    overflow = []
    try:
        with torch.no_grad():
            eng = make_engine(model, n)
            L0 = min(len(s.generated) for s in st)
            tok = torch.tensor([s.generated[:L0] for s in st], dtype=torch.long, device=dev)
            seg = torch.tensor([s.seg[:L0] for s in st], dtype=torch.long, device=dev)
            logits = eng.prefill(tok, seg)
            for s in st:
                s.consumed = L0
            while True:
                logits_np = None
                for i, s in enumerate(st):
                    if s.done:
                        continue
                    if len(s.generated) >= max_dec_inp_len:      # window slides: positions restart, the recurrent state is void
                        s.done = True
                        overflow.append(i)
                        continue
                    if s.consumed < len(s.generated):
                        continue
                    if logits_np is None:
                        logits_np = logits.cpu().numpy()
                        if getattr(eng, 'persist', None) is not None:
                            eng.check_persistent()
                    while True:                                  # a rejected sample re-derives probs from the same logits (reference: `continue`)
                        probs = temperature(logits_np[i].copy(), temp, inadmissibles=inadmissibles)
                        if s.offer(int(samplers[i](probs)), event2idx, idx2event, skip_check, max_events):
                            break
                if all(s.done for s in st):
                    break
                nxt_tok = [s.generated[s.consumed] if s.consumed < len(s.generated) else pad for s in st]
                nxt_seg = [s.seg[s.consumed] if s.consumed < len(s.seg) else 1 for s in st]
                for s in st:
                    if s.consumed < len(s.generated):
                        s.consumed += 1
                logits = eng.step(torch.tensor(nxt_tok, dtype=torch.long, device=dev), torch.tensor(nxt_seg, dtype=torch.long, device=dev))
    finally:
        model.train(was_training)
    out = [s.result() for s in st]
    for i in overflow:       # rare: hand the stream to the reference-shaped single-stream loop (full-window forward per token)
        out[i] = _resume_windowed(model, event2idx, idx2event, st[i], max_events, skip_check, temp, inadmissibles, samplers[i])
    return out


def _resume_windowed(model, event2idx, idx2event, s, max_events, skip_check, temp, inadmissibles, sampler):
    dev = next(model.parameters()).device
    s.done = False
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            while not s.done:
                dec_input = torch.tensor([s.generated[-max_dec_inp_len:]], dtype=torch.long, device=dev)
                dec_seg = torch.tensor([s.seg[-max_dec_inp_len:]], dtype=torch.long, device=dev)
                kw = {'attn_kwargs': {'omit_feature_map_draw': True}} if model.kind == 'performer' else {}
                logits_np = model(dec_input, seg_inp=dec_seg, keep_last_only=True, **kw)[0].cpu().numpy().copy()
                while True:
                    probs = temperature(logits_np.copy(), temp, inadmissibles=inadmissibles)
                    if s.offer(int(sampler(probs)), event2idx, idx2event, skip_check, max_events):
                        break
    finally:
        model.train(was_training)
    return s.result()


@torch.no_grad()
def generate_streams(model, prompt_tok, prompt_seg, n_new, temp=1.1, top_p=0.9, greedy=False, seed=0, seg_value=1, use_graph=True, chains=None):
    """BASELINE configs[3]: n parallel streams in lock-step (grammar checks off => fixed token count).  Everything stays
    on the GPU: recurrent/KV state, positions, sampling, token buffer.  One decode step is ~64 small DEPENDENT launches (one where the engine
    has the one-launch step), so the step (sample -> append -> embed -> 12 layers -> logits) is captured ONCE in a hipGraph and replayed per
    token (replay.StepReplayer with a fixed step count: every replay is enqueued without reading anything back).  `chains`: None or 1; the
    mode that split the streams over several graphs on several HIP streams is gone (slower at every split).
    Returns int64 [n, T0 + n_new]."""
    if chains not in (None, 1):
        raise ValueError('generate_streams: chains=%r: the multi-chain mode (streams split over several graphs / HIP streams) was removed' % (chains,))
    n, T0 = prompt_tok.shape
    dev = prompt_tok.device
    U = uniform_table(max(n_new, 1), n, seed, dev)
    eng = make_engine(model, n)
    out = torch.empty(n, T0 + n_new, dtype=torch.long, device=dev)
    out[:, :T0] = prompt_tok
    seg_col = torch.full((n,), seg_value, dtype=torch.long, device=dev)
    logits_buf = eng.prefill(prompt_tok.contiguous(), prompt_seg.contiguous()).clone()
    if not greedy:
        # all loop state on the device inside OUR kernels: the sampler reads u[step[r], r], writes the token into out[r, T0 + step[r]] and
        # advances step[r]; the embedding takes position (T0 - 1) + step[r]; the logits GEMM writes straight into logits_buf
        # (5 fewer launches per token than the torch index_select / scatter_ / add_ / copy_ version below).
        step_ctr = torch.zeros(n, dtype=torch.long, device=dev)
        eng.pos_dev, eng.dev_pos0, eng.pos_auto = step_ctr, T0 - 1, False
        nxt_buf = torch.empty(n, dtype=torch.long, device=dev)

        if eng.persist is not None and os.environ.get('EMO_PD_SAMPLER', '1') != '0':
            # one launch per token: the draw runs inside the persistent step (the same device code as emo_sample_nucleus_step)
            eng.load_logits(logits_buf)
            seg_p = torch.zeros(eng.n_pad, dtype=torch.long, device=dev)
            seg_p[:n] = seg_col

            def one_step():
                eng.step_sampled(seg_p, temp, top_p, U, step_ctr, out, T0, nxt_buf, T0 - 1)
        else:
            def one_step():
                ops.sample_nucleus_step(logits_buf, temp, top_p, U, step_ctr, seq=out, col0=T0, out=nxt_buf)
                eng.step(nxt_buf, seg_col, dev_pos=True, logits_out=logits_buf)
    else:
        step_idx = torch.zeros(1, dtype=torch.long, device=dev)

        def one_step():
            u = U.index_select(0, step_idx).view(n)
            nxt = sample_on_device(logits_buf, temp, top_p, u, greedy)
            out.scatter_(1, (step_idx + T0).expand(n, 1), nxt.view(n, 1))
            logits_buf.copy_(eng.step(nxt, seg_col, dev_pos=True))
            step_idx.add_(1)
    rp = StepReplayer(one_step, dev)
    rp.run(0, n_new, use_graph=use_graph)
    if os.environ.get('EMO_GEN_TIMING') and rp.replayed[0]:      # diagnostics: host time to ENQUEUE the replays vs time until the GPU is done
        steps, t_enq = rp.replayed
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        print('[gen timing] enqueue %.3f ms/step, total %.3f ms/step' % (1e3 * t_enq / steps, 1e3 * (t_enq + time.perf_counter() - t1) / steps))
    eng.check_persistent()
    return out


# ------------------------------------------------------------------------------------------------ device loop (stage 2, grammar on)
# Mirrors of include/emo_hip.h (emo_grammar_step, kinds ACC / ACC_WINDOW): per-token event bits, per-stream parameter and state words, stream status.
ACC_EV_BEAT, ACC_EV_TRACK_LS, ACC_EV_PAD, ACC_EV_EOS = 1, 2, 4, 8
ACC_P_TARGET_BARS, ACC_P_MAX_EVENTS, ACC_P_SKIP_CHECK, ACC_P_BAR0, ACC_P_N_BARS = range(5)
ACC_S_STATUS, ACC_S_LEN, ACC_S_CONSUMED, ACC_S_BARS, ACC_S_CUR_POS, ACC_S_FAILED, ACC_S_DRAWS, ACC_S_ACCEPTED = range(8)
ACC_RUNNING, ACC_DONE, ACC_STUCK, ACC_WINDOW, ACC_OUT_OF_DRAWS, ACC_OVERFLOW = range(6)


def acc_event_tables(idx2event, V):
    """-> (flags int32 [V], beat positions int32 [V]): the tests _Stream.offer makes of an event name, per token id ('Beat' in e with
    beat_position, e == 'Track_LeadSheet', e == 'PAD_None', e == 'EOS_None').  Ids without an event get no bits."""
    flags, beat = np.zeros(V, np.int32), np.zeros(V, np.int32)
    for i in range(V):
        e = event_name(idx2event, i)
        if e is None:
            continue
        f = 0
        if 'Beat' in e:
            f |= ACC_EV_BEAT
            beat[i] = beat_position(e)
        if e == 'Track_LeadSheet':
            f |= ACC_EV_TRACK_LS
        if e == 'PAD_None':
            f |= ACC_EV_PAD
        if e == 'EOS_None':
            f |= ACC_EV_EOS
        flags[i] = f
    return flags, beat


def pack_lead_sheets(lead_sheets):
    """n lead sheets (lists of bars, each a list of ids) -> (tokens int64, offsets int32, first-bar index per stream, bar count per stream,
    longest bar): bar j of stream i is tokens[offsets[bar0[i] + j] : offsets[bar0[i] + j + 1]] (emo_hip.h: EMO_GRAMMAR_ACC)."""
    toks, offs, bar0, nbars = [], [], [], []
    for lead in lead_sheets:
        bar0.append(len(offs))
        nbars.append(len(lead))
        for b in lead:
            offs.append(len(toks))
            toks.extend(int(t) for t in b)
        offs.append(len(toks))
    longest = max([len(b) for lead in lead_sheets for b in lead] or [0])
    return np.array(toks or [0], np.int64), np.array(offs, np.int32), bar0, nbars, longest


def tempo_ban(event2idx, tempo, tolerance=20):
    """The ids of the tempo events further than `tolerance` from `tempo`: every key of event2idx that contains 'Tempo' and not 'Conti' and
    whose trailing integer differs from tempo by more than tolerance.  As `banned` of generate_accompaniments (or `inadmissibles` of the host
    loops) it keeps the drawn tempi within tempo +- tolerance."""
    return sorted(i for e, i in event2idx.items() if 'Tempo' in e and 'Conti' not in e and abs(int(e.rsplit('_', 1)[-1]) - tempo) > tolerance)


def _refuse(model, inadmissibles):
    if inadmissibles is not None:
        raise ValueError('generate_accompaniments: `inadmissibles` is not supported by the device grammar')
    check_vocab('generate_accompaniments', model.n_token)


class _GaveUp(Exception):
    """The one-launch decode step gave up (emo_*_decode_step: its workgroups were not all resident in time)."""


def _stream_result(status, ids, out_of_draws, overflow, still_running):
    """Status word and ids so far of a stream that is not at the window -> what _Stream.result() gives (DONE: generated[:-1], STUCK:
    generated), or an EmoError with the caller's text for an exhausted uniform table, a row / table limit, or a stream still running."""
    if status == ACC_DONE:
        return ids[:-1]
    if status == ACC_STUCK:
        return ids
    return EmoError('generate_accompaniments: ' + (out_of_draws if status == ACC_OUT_OF_DRAWS else overflow if status == ACC_OVERFLOW else still_running))


class AccompanimentLoop(GrammarLoop):
    """Device state of generate_accompaniments: the decode engine (prefilled with the common prefix, positions on the device), the logits of
    the last step, the uniform table, the grammar tables, the packed lead sheets, per-stream parameters / state and token / segment rows, and
    the running count; one_step() = emo_grammar_step (kind ACC) + the engine step.  scores=True: the grammar launch also records every accepted
    draw's log-probability, rank and entropy in self.score_tables (ops.draw_score_tables: laid out like seq, sentinels wherever a token was
    given, not drawn: primer, injected bars, Track_Full); a WindowedLoop takes the rows over at the hand-off and goes on recording; scores()
    reads them.  The streams that _resume_windowed finishes on the host (window='host') keep sentinels from the hand-off on: its draws are
    NumPy's, made from host probabilities, and are not recorded."""

    def __init__(self, model, event2idx, idx2event, lead_sheets, primers, max_events=10000, skip_check=False, max_bars=None, temp=1.2, top_p=0.9,
                 seed=0, n_u=None, persistent=True, redraw=True, scores=False, banned=None):
        self._load_jobs(model, event2idx, idx2event, lead_sheets, primers, max_events, skip_check, max_bars, temp, top_p, None, banned)
        n, dev, V = self.n, self.dev, model.n_token
        self.U = uniform_table(int(n_u or 4 * self.W), n, seed, dev)
        self.tok = torch.zeros(n, dtype=torch.int64, device=dev)
        self.segv = torch.ones(n, dtype=torch.int64, device=dev)
        self.logits = torch.empty(n, V, dtype=torch.float32, device=dev)
        self._build_block(ops.GRAMMAR_ACC, scores, self.job_controls, **self._block_fields(n))
        self.windowed = None
        with torch.no_grad():
            eng = self._make_engine(n, persistent, redraw)
            self.logits.copy_(eng.prefill(self.seq[:, :self.L0].contiguous(), self.segs[:, :self.L0].contiguous()))
            eng.pos_dev.zero_()
            eng.dev_pos0, eng.pos_auto = self.L0, True          # position = L0 + pos_dev[r], advanced by the engine
        self.eng = eng
        pe = model.pe.pe.shape[0] if model.use_pe else self.W
        self.bound = min(self.W, pe)           # the engine never runs a step at a position >= bound (the one-launch GPT-2 step would clamp it)
        self.pos = self.L0                     # host count of the engine position (every row advances one per step)

    def _load_jobs(self, model, event2idx, idx2event, lead_sheets, primers, max_events, skip_check, max_bars, temp, top_p, consumed, banned=None):
        """n, model, dev, W and the draw parameters (job_controls: gen_loop.draw_controls of temp / top_p / banned, each one value for all streams
        or one per stream, checked before anything is allocated; temp / top_p: the launch's scalars); the grammar tables, the packed lead sheets and, per stream, its _Stream and its token / segment
        rows, parameters and state on the device, state[CONSUMED] = `consumed` (None: the shortest prompt's length L0, the prefix a prefill
        takes); the running count."""
        n = self.n = len(lead_sheets)
        assert n == len(primers) and n > 0
        _refuse(model, None)
        ctl = self.job_controls = draw_controls('generate_accompaniments', n, model.n_token, banned, temp, top_p)
        self.model, self.temp, self.top_p = model, ctl.temp, ctl.top_p
        self.max_events = int(max_events)
        self.W = int(max_dec_inp_len)                 # read at call time (tests lower it)
        dev = self.dev = next(model.parameters()).device
        self.streams = [_Stream(event2idx, lead_sheets[i], primers[i], max_bars) for i in range(n)]
        V = model.n_token
        self._upload_events(*acc_event_tables(idx2event, V))
        toks, offs, bar0, nbars, longest = pack_lead_sheets(lead_sheets)
        self.lead_tok, self.lead_off = self._to_device(toks, offs)
        self.track_full, self.pad = event2idx['Track_Full'], event2idx.get('PAD_None', 0)
        self.track_leadsheet, self.primer_lens = event2idx['Track_LeadSheet'], [len(p) for p in primers]      # (what a RebaseLoop cuts by)
        self.longest_bar = longest
        lens = [len(s.generated) for s in self.streams]
        width = max(self.W, max(lens)) + longest + 2              # an injected bar + Track_Full always fit behind an accepted word
        seq, segs = np.zeros((n, width), np.int64), np.zeros((n, width), np.int64)
        params = np.zeros((n, ops.ACC_PARAM_WORDS), np.int32)
        state = np.zeros((n, ops.ACC_STATE_WORDS), np.int32)
        self.L0 = min(lens)
        for i, s in enumerate(self.streams):
            seq[i, :lens[i]], segs[i, :lens[i]] = s.generated, s.seg
            params[i, [ACC_P_TARGET_BARS, ACC_P_MAX_EVENTS, ACC_P_SKIP_CHECK, ACC_P_BAR0, ACC_P_N_BARS]] = (s.target_bars, max_events, bool(skip_check),
                                                                                                            bar0[i], nbars[i])
            state[i, [ACC_S_STATUS, ACC_S_LEN, ACC_S_CONSUMED]] = (ACC_DONE if s.done else ACC_RUNNING), lens[i], self.L0 if consumed is None else consumed
        self.len0 = np.array(lens)
        self.seq, self.segs, self.params, self.state = self._to_device(seq, segs, params, state)
        self.running = torch.tensor([int((state[:, ACC_S_STATUS] == ACC_RUNNING).sum())], dtype=torch.int32, device=dev)

    def _block_fields(self, rows):
        """The fields of the grammar launch's block that kinds ACC and ACC_QUEUE share, for a model batch of `rows` rows."""
        return dict(n_rows=rows, n_token=self.model.n_token, ld_u=self.n, temperature=self.temp, top_p=self.top_p, max_len=self.W,
                    track_full=self.track_full, pad=self.pad, logits=self.logits, u_steps=self.U, ev_flags=self.ev_flags,
                    ev_beat=self.ev_beat, lead_tok=self.lead_tok, lead_off=self.lead_off, params=self.params, state=self.state, seq=self.seq,
                    segs=self.segs, tok_out=self.tok, seg_out=self.segv, running=self.running)

    def _make_engine(self, rows, persistent, redraw):
        """The decode engine of `rows` rows whose positions and cache end at the window."""
        if self.model.kind == 'performer':
            eng = PerformerDecodeEngine(self.model, rows, redraw=redraw, persistent=persistent)
            eng.max_len = self.W
            return eng
        return GPT2DecodeEngine(self.model, rows, max_len=self.W, persistent=persistent)

    def one_step(self):
        self.grammar()
        self.eng.step(self.tok, self.segv, dev_pos=True, logits_out=self.logits)

    def _live(self):
        """Running count (synchronises); raises _GaveUp when the one-launch step gave up."""
        if self.eng.persist is not None:
            try:
                self.eng.check_persistent()
            except EmoError as e:
                raise _GaveUp(str(e))
        return int(self.running.item())

    def run(self, use_graph=True, steps_per_graph=None):
        """Steps until every stream has left RUNNING; the running count is read once per replay (per step without graphs).  A k-step replay
        runs only while it keeps the position below `bound`; at the bound one more grammar step runs alone (a stream still running there
        reaches the window in it)."""
        with torch.no_grad():
            self.pos = self._replay(self.pos, self.bound, use_graph, steps_per_graph)
            if self._live() > 0:
                self.grammar()
            torch.cuda.synchronize()

    def steps(self):
        return self.pos - self.L0

    def accepted_tokens(self):
        return int(self.state[:, ACC_S_ACCEPTED].sum().item())

    def counts(self):
        st = self.state[:, ACC_S_STATUS].cpu().numpy()
        return {'finished': int((st == ACC_DONE).sum()), 'stuck': int((st == ACC_STUCK).sum()), 'window': int((st == ACC_WINDOW).sum()),
                'other': int(((st != ACC_DONE) & (st != ACC_STUCK) & (st != ACC_WINDOW)).sum())}

    def handed_off(self, i, state=None, seq=None, segs=None):
        """Stream i as the host grammar continues it: its _Stream rebuilt from the device state (host copies may be passed in)."""
        state = self.state.cpu().numpy() if state is None else state
        seq = self.seq[i].cpu().numpy() if seq is None else seq[i]
        segs = self.segs[i].cpu().numpy() if segs is None else segs[i]
        s, ln = self.streams[i], int(state[i, ACC_S_LEN])
        s.generated, s.seg = [int(t) for t in seq[:ln]], [int(t) for t in segs[:ln]]
        s.generated_bars, s.cur_pos, s.failed_cnt = (int(state[i, w]) for w in (ACC_S_BARS, ACC_S_CUR_POS, ACC_S_FAILED))
        s.consumed = int(state[i, ACC_S_CONSUMED])
        return s

    def results(self, event2idx, idx2event, max_events, skip_check, seed, window='host', rebase_keep=None, use_graph=True):
        """Per stream what _Stream.result() gives: DONE -> generated[:-1], STUCK -> generated; WINDOW -> the stream rebuilt from the device
        state and finished by _resume_windowed with nucleus(probs, top_p, rng=RandomState([seed, i])), or with window='device' finished
        together with the other WINDOW streams by a WindowedLoop (kept in self.windowed); an exhausted uniform table (or a row / position
        limit) -> an EmoError in the stream's slot."""
        state, seq, segs = self.state.cpu().numpy(), self.seq.cpu().numpy(), self.segs.cpu().numpy()
        past = {}
        if window == 'device' and (state[:, ACC_S_STATUS] == ACC_WINDOW).any():
            self.windowed = WindowedLoop(self, seed)
            self.windowed.run()
            past = dict(zip(self.windowed.idx, self.windowed.results()))
        elif window == 'rebase' and (state[:, ACC_S_STATUS] == ACC_WINDOW).any():
            # re-anchored on a bar and continued with cached one-token steps (RebaseLoop, kept in self.windowed like the WindowedLoop)
            self.windowed = RebaseLoop(self, seed, rebase_keep)
            self.windowed.run(use_graph=use_graph)
            past = dict(zip(self.windowed.idx, self.windowed.results()))
        out = []
        for i, s in enumerate(self.streams):
            st, ln = int(state[i, ACC_S_STATUS]), int(state[i, ACC_S_LEN])
            if st == ACC_WINDOW and i in past:
                out.append(past[i])
            elif st == ACC_WINDOW:
                s = self.handed_off(i, state, seq, segs)
                rs = np.random.RandomState([seed, i])
                ctl = self.job_controls                      # the stream keeps its controls: the host loop's `inadmissibles` is its ban
                out.append(_resume_windowed(self.model, event2idx, idx2event, s, max_events, skip_check, ctl.temp_at(i),
                                            list(ctl.bans[i]) if ctl.bans[i] else None,
                                            lambda probs, rs=rs, p=ctl.top_p_at(i): nucleus(probs, p, rng=rs)))
            else:
                out.append(_stream_result(st, [int(t) for t in seq[i, :ln]], 'stream %d used all %d uniforms of its table' % (i, self.U.shape[0]),
                                          'stream %d: token row or lead-sheet table too short' % i,
                                          'stream %d still running at position %d (positional table / cache end)' % (i, self.pos)))
        return out

    def scores(self, results):
        """-> per stream, aligned with `results` (what results() returned): {'logp', 'rank', 'entropy'} numpy arrays with one entry per id of
        the stream's result (NaN / -1 where the id was given, and from the hand-off on where the host finished the stream), or None where the
        result is an error.  Needs scores=True."""
        own = self.score_arrays()
        past, at = own, {}
        if self.windowed is not None and self.windowed.score_tables is not None:
            past = self.windowed.score_arrays()
            at = {i: j for j, i in enumerate(self.windowed.idx)}
        out = []
        for i, ids in enumerate(results):
            if isinstance(ids, Exception):
                out.append(None)
                continue
            tabs, row = (past, at[i]) if i in at else (own, i)
            sc = {}
            for k, t in tabs.items():
                a = np.full(len(ids), -1 if k == 'rank' else np.nan, dtype=t.dtype)
                n = min(len(ids), t.shape[1])
                a[:n] = t[row, :n]
                sc[k] = a
            out.append(sc)
        return out


class AccompanimentQueue(AccompanimentLoop):
    """AccompanimentLoop for more jobs than rows: `slots` rows of the model batch (one decode engine of that many rows) work through
    len(lead_sheets) queued jobs.  one_step() = emo_grammar_step (kind ACC_QUEUE) + the restart of the admitted rows' FAVOR+ state (Performer
    only: emo_favor_state_reset on the launch's row_reset flags; a GPT-2 row restarts by being fed position 0) + the engine step: a slot whose
    job ends takes the next job inside the grammar launch, so the replayed graphs go on and the running count stays the only thing read back.
    There is no prefill: the first launch admits the first jobs and every prompt token goes through the one-token step, at the position the
    grammar launch writes into the engine's device position array (pos_auto False, dev_pos0 0: generate_streams' mode).  Job j draws from column
    j of the uniform table, whatever slot it lands in; all jobs run under the engine's one set of feature maps.  A job that reaches the window
    ends with WINDOW and frees its slot; results() finishes it as it finishes a lock-step stream.  The lock-step loop's host position bound
    does not apply: the per-job bound is the kernel's (mem_rows = the window; a positional table with fewer rows is refused here).  results() /
    scores() / handed_off() are AccompanimentLoop's, per job; job_steps: the launches each finished job held a slot; launches: the launches run()
    queued (a k-step replay ends up to k - 1 launches past the drain)."""

    def __init__(self, model, event2idx, idx2event, lead_sheets, primers, slots, max_events=10000, skip_check=False, max_bars=None, temp=1.2,
                 top_p=0.9, seed=0, n_u=None, persistent=True, redraw=True, scores=False, banned=None):
        slots = self.slots = int(slots)
        if slots < 1:
            raise ValueError('slots must be at least 1 (got %d)' % slots)
        # CONSUMED 1 is what an admission sets: the first token goes out with it
        self._load_jobs(model, event2idx, idx2event, lead_sheets, primers, max_events, skip_check, max_bars, temp, top_p, 1, banned)
        n, dev, V = self.n, self.dev, model.n_token
        if model.use_pe and model.pe.pe.shape[0] < self.W:
            raise EmoError('generate_accompaniments(slots=): the positional table has %d rows, fewer than the window of %d tokens'
                           % (model.pe.pe.shape[0], self.W))
        self.bound = self.W
        self.U = uniform_table(int(n_u or 4 * self.W), n, seed, dev)
        self.tok = torch.full((slots,), self.pad, dtype=torch.int64, device=dev)
        self.segv = torch.ones(slots, dtype=torch.int64, device=dev)
        self.logits = torch.zeros(slots, V, dtype=torch.float32, device=dev)
        self.slot_job = torch.full((slots,), -1, dtype=torch.int32, device=dev)
        self.queue_head = torch.zeros(1, dtype=torch.int32, device=dev)
        self.row_reset = torch.zeros(slots, dtype=torch.int32, device=dev)
        self.job_steps_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self.windowed = None
        with torch.no_grad():
            eng = self.eng = self._make_engine(slots, persistent, redraw)
            eng.pos_dev.zero_()
            eng.dev_pos0, eng.pos_auto = 0, False                # position = pos_dev[b], written by the grammar launch
            self.state_table = eng.start_empty() if model.kind == 'performer' else None
        self._build_block(ops.GRAMMAR_ACC_QUEUE, scores, self.job_controls, n_jobs=n, mem_rows=self.bound, slot_job=self.slot_job, queue_head=self.queue_head,
                          mem_lens=eng.pos_dev, row_reset=self.row_reset, job_steps=self.job_steps_dev, **self._block_fields(slots))
        # no job is fed more tokens than the window holds, so the queue is drained before this many launches whatever the slots do: a budget
        # for the replayer, not a limit that is meant to bind (the per-job limit is the kernel's WINDOW)
        self.budget = n * self.W + 2
        self.launches = self.pos = 0

    def model_step(self):
        """What follows the grammar launch: the restart of the rows it flagged (Performer), then the engine step on the tokens, segments and
        positions it wrote."""
        if self.state_table is not None:
            ops.favor_state_reset(self.state_table, self.slots, self.eng.S[0][0].numel(), self.eng.z[0][0].numel(), self.row_reset)
        self.eng.step(self.tok, self.segv, dev_pos=True, logits_out=self.logits)

    def one_step(self):
        self.grammar()
        self.model_step()

    def run(self, use_graph=True, steps_per_graph=None):
        """Launches until the running count is 0; it is read once per replay (per step without graphs)."""
        with torch.no_grad():
            self.launches = self.pos = self._replay(self.launches, self.budget, use_graph, steps_per_graph)
            torch.cuda.synchronize()
            if self._live() > 0:
                raise EmoError('AccompanimentQueue: %d jobs still running after %d launches' % (self._live(), self.launches))

    def steps(self):
        return self.launches

    def job_steps(self):
        """-> per job, the launches it held a slot (0 for a job that was closed before the run)."""
        return [int(x) for x in self.job_steps_dev.cpu().tolist()]


WINDOW_TAG = 0x57494E                  # the windowed phase's uniform table is seeded with (seed, this tag): never the in-window table's seed


def window_compaction(live):
    """The compaction rule of WindowedLoop.  live: one bool per row of the current batch, in batch order -> the positions the batch continues
    on: the live ones, in order, once they are at most half of the rows; every position until then (a smaller batch means new GEMM shapes and a
    fresh gather of the windows, so it has to pay: one long stream must not carry 31 finished rows through every forward)."""
    keep = [p for p, x in enumerate(live) if x]
    return keep if 2 * len(keep) <= len(live) else list(range(len(live)))


class WindowedLoop(GrammarLoop):
    """The ACC_WINDOW streams of a finished AccompanimentLoop, continued together on the device (the reference's sliding window, inference.py
    :252-277, which _resume_windowed runs one stream and one host round trip at a time).  One step = one forward over the streams' last W tokens,
    model(win_tok, seg_inp=win_seg, keep_last_only=True) on [m, W] — positions restart at 0, so nothing carries over between steps — and
    emo_grammar_step (kind ACC_WINDOW): the draw, the in-launch redraws, the grammar, and the next window of every stream still running.  Streams are indexed
    by their place j among the WINDOW streams (self.idx[j] = the stream of the first loop): seq / segs [m0, width] (copies, wide enough for the
    whole piece), params / state [m0, 8] (status RUNNING again, draw counter 0), the uniform table U [n_u, m0] of this phase alone, seeded with
    (seed, WINDOW_TAG).  The host reads the running count once every `steps_per_poll` steps (EMO_GEN_GRAPH_STEPS, default 16; steps a stream
    does not need are no-ops for it) and then applies window_compaction: self.rows (int32, stream j of each batch row) shrinks, nothing else
    moves.  self.batch_rows: the row count of every step run.  The forward is the model's eager one (not captured in a hipGraph: DESIGN.md)."""

    def __init__(self, loop, seed, n_u=None, steps_per_poll=None):
        self.loop, self.model, self.dev = loop, loop.model, loop.dev
        self.W, self.temp, self.top_p = loop.W, loop.temp, loop.top_p
        dev, W = self.dev, self.W
        state = loop.state.cpu().numpy()
        self.idx = [i for i in range(loop.n) if state[i, ACC_S_STATUS] == ACC_WINDOW]
        m0 = self.m0 = len(self.idx)
        assert m0 > 0, 'no stream reached the window'
        self.k = graph_steps(steps_per_poll)
        sel = torch.tensor(self.idx, dtype=torch.long, device=dev)
        len0 = state[self.idx, ACC_S_LEN].astype(np.int64)
        self.len0 = len0
        w0 = loop.seq.shape[1]
        width = max(w0, int(len0.max()) + loop.max_events + loop.longest_bar + 2)     # the whole piece: max_events, the longest bar and 2 past the handoff
        self.seq = torch.zeros(m0, width, dtype=torch.int64, device=dev)
        self.segs = torch.zeros(m0, width, dtype=torch.int64, device=dev)
        self.seq[:, :w0], self.segs[:, :w0] = loop.seq[sel], loop.segs[sel]
        self.params = loop.params[sel].contiguous()
        self.state = loop.state[sel].contiguous()
        self.state[:, ACC_S_STATUS] = ACC_RUNNING
        self.state[:, ACC_S_DRAWS] = 0
        self.accepted0 = int(self.state[:, ACC_S_ACCEPTED].sum().item())
        self.running = torch.tensor([m0], dtype=torch.int32, device=dev)
        # max_events draws can be accepted at most; every rejected run before an acceptance is shorter than 256 Beats plus the PAD / early-EOS
        # draws, which a trained model all but never makes: as many again, and one STUCK run
        self.U = uniform_table(int(n_u or 2 * loop.max_events + 256), m0, (int(seed) * 0x9E3779B1 + WINDOW_TAG) & 0x7FFFFFFFFFFFFFFF, dev)
        self.win_tok = torch.zeros(m0, W, dtype=torch.int64, device=dev)
        self.win_seg = torch.zeros(m0, W, dtype=torch.int64, device=dev)
        self.logits = torch.zeros(m0, self.model.n_token, dtype=torch.float32, device=dev)
        self.fwd_kw = {'attn_kwargs': {'omit_feature_map_draw': True}} if self.model.kind == 'performer' else {}
        self.batch_rows, self.steps, self.seconds = [], 0, 0.0
        # the windowed step's block, written once for the full batch; _set_rows keeps n_rows / rows current
        self._build_block(ops.GRAMMAR_ACC_WINDOW, loop.score_tables is not None, loop.job_controls.take(self.idx), n_rows=m0, n_token=self.model.n_token, ld_u=m0,
                          temperature=self.temp, top_p=self.top_p, window=W, track_full=loop.track_full, logits=self.logits, u_steps=self.U,
                          ev_flags=loop.ev_flags, ev_beat=loop.ev_beat, lead_tok=loop.lead_tok, lead_off=loop.lead_off, params=self.params,
                          state=self.state, seq=self.seq, segs=self.segs, win_tok=self.win_tok, win_seg=self.win_seg, running=self.running)
        # the first loop's recorded draws travel with the token rows; the windowed launch goes on recording behind them
        for k, t in (self.score_tables or {}).items():
            t[:, :w0] = loop.score_tables[k][sel]
        self._set_rows(list(range(m0)))

    def _set_rows(self, rows):
        """The batch continues on these streams: rows [m] and their windows seq / segs[j, LEN - W .. LEN), gathered on the device."""
        if not rows or len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= self.m0:
            raise EmoError('WindowedLoop: batch rows %r are not distinct streams of 0 .. %d' % (rows, self.m0 - 1))
        self.m = len(rows)
        self.rows_host = list(rows)
        self.rows = torch.tensor(rows, dtype=torch.int32, device=self.dev)
        # the only fields that change: logits[:m], win_tok[:m] and win_seg[:m] keep their base addresses.  The block is read at call time and this
        # loop is eager (no captured launch holds the old values), so the next one_step runs on the new rows.
        ops.block_set(self._gargs, self._gheld, n_rows=self.m, rows=self.rows)
        r = self.rows.long()
        col = (self.state[r, ACC_S_LEN].long() - self.W).view(-1, 1) + torch.arange(self.W, device=self.dev).view(1, -1)
        self.win_tok[:self.m] = self.seq[r].gather(1, col)
        self.win_seg[:self.m] = self.segs[r].gather(1, col)

    def one_step(self):
        m = self.m
        self.logits[:m].copy_(self.model(self.win_tok[:m], seg_inp=self.win_seg[:m], keep_last_only=True, **self.fwd_kw))
        ops.grammar_step(self._gargs)
        self.batch_rows.append(m)
        self.steps += 1

    def poll(self):
        """Running count (synchronises), then the compaction rule (window_compaction alone decides).  -> streams still running."""
        live = int(self.running.item())
        if live > 0:
            status = self.state[:, ACC_S_STATUS].cpu().numpy()
            keep = window_compaction([status[j] == ACC_RUNNING for j in self.rows_host])
            if len(keep) < self.m:
                self._set_rows([self.rows_host[p] for p in keep])
        return live

    def run(self, max_steps=None):
        """Steps until no stream is RUNNING (or `max_steps` steps have run: benchmarks), polling every k steps."""
        t0 = time.perf_counter()
        with scoring.eval_mode(self.model), torch.no_grad():
            while max_steps is None or self.steps < max_steps:
                for _ in range(self.k if max_steps is None else min(self.k, max_steps - self.steps)):
                    self.one_step()
                if self.poll() == 0:
                    break
            torch.cuda.synchronize()
        self.seconds += time.perf_counter() - t0

    def accepted_draws(self):
        return int(self.state[:, ACC_S_ACCEPTED].sum().item()) - self.accepted0

    def results(self):
        """Per WINDOW stream, in the order of self.idx, what _Stream.result() gives (or an EmoError, as AccompanimentLoop.results)."""
        state, seq = self.state.cpu().numpy(), self.seq.cpu().numpy()
        out = []
        for j, i in enumerate(self.idx):
            st, ids = int(state[j, ACC_S_STATUS]), [int(t) for t in seq[j, :int(state[j, ACC_S_LEN])]]
            out.append(_stream_result(st, ids, 'stream %d used all %d uniforms of its windowed table' % (i, self.U.shape[0]),
                                      'stream %d: token row or lead-sheet table too short past the window' % i,
                                      'stream %d still running after %d windowed steps' % (i, self.steps)))
        return out


REBASE_TAG = 0x524542                  # a rebase phase's uniform table is seeded with (seed, this tag, phase): never WINDOW_TAG's or the in-window seed
ACC_BAR_TOO_LONG = 6                   # emo_hip.h: EMO_REBASE_BAR_TOO_LONG, the status emo_acc_rebase alone writes


def rebase_plan(seq_row, n, primer_len, track_leadsheet, keep, W, longest_bar):
    """The re-anchoring rule of window='rebase' for one stream, on the host (emo_acc_rebase is the same rule on the device).  seq_row[:n]: the
    stream's tokens, primer_len primer ids followed by bars that each open with track_leadsheet (a drawn one counts like an injected one).
    -> (b, new_len): the context continues as seq_row[:primer_len] + seq_row[b:n], new_len = primer_len + n - b tokens; b is the smallest bar
    start that leaves at most `keep` tokens, else the last bar start when that leaves at most W - longest_bar - 2 (an injected bar and
    Track_Full still fit below the window); else ACC_BAR_TOO_LONG (an int: a bar longer than the window).  b - primer_len tokens are dropped:
    the stream's max_events goes down by as many (rebase_max_events)."""
    P, n = int(primer_len), int(n)
    starts = [i for i in range(P, n) if int(seq_row[i]) == track_leadsheet]
    fit = [i for i in starts if P + (n - i) <= keep]
    if fit:
        return fit[0], P + n - fit[0]
    if starts and P + (n - starts[-1]) <= W - longest_bar - 2:
        return starts[-1], P + n - starts[-1]
    return ACC_BAR_TOO_LONG


def rebase_max_events(max_events, b, primer_len):
    """max_events of a re-anchored stream: the reference's whole-piece limit len(generated) > max_events, counted in the new context's indices."""
    return int(max_events) - (int(b) - int(primer_len))


def rebase_stitch(primer, archive, tail):
    """The piece so far of a re-anchored stream: its primer, the tokens (or score cells) its rebases dropped, in order, and its current context
    behind the primer."""
    return list(primer) + list(archive) + list(tail)


def check_rebase_keep(rebase_keep, W, longest_primer, longest_bar):
    """rebase_keep of generate_accompaniments -> the checked value (None: W // 2).  ValueError unless the longest primer, a Track_LeadSheet and
    one token more fit it and a context of that size leaves room for the longest lead-sheet bar and its two Track marks below the window."""
    keep = W // 2 if rebase_keep is None else rebase_keep
    if isinstance(keep, bool) or not isinstance(keep, (int, np.integer)):
        raise ValueError('rebase_keep must be an integer (got %r)' % (rebase_keep,))
    lo, hi = int(longest_primer) + 2, W - int(longest_bar) - 2
    if not lo <= keep <= hi:
        raise ValueError('rebase_keep = %d is outside [%d, %d] = [len(primer) + 2, window - longest bar - 2]' % (keep, lo, hi))
    return int(keep)


class RebaseLoop(GrammarLoop):
    """The ACC_WINDOW streams of a finished AccompanimentLoop / AccompanimentQueue, continued by re-anchoring (window='rebase').  A phase =
    emo_acc_rebase (every WINDOW row drops its oldest whole bars, keeps its primer and becomes a context of at most `keep` tokens: rebase_plan),
    one variable-length prefill of the batch (prefill(lens=)), then an ordinary in-window run on the shorter rows: emo_grammar_step of kind ACC
    (unchanged) + the engine's one-token step, replayed by the shared replay driver until the longest row reaches the bound.  Rows still
    RUNNING there are shorter than the row that reached it; they are marked WINDOW and re-anchored with it (a rebase of a row below `keep`
    moves nothing).  Phases repeat while any row is at WINDOW.  Streams are indexed by their place j among the WINDOW streams (self.idx[j] = the
    stream of the first loop).  Rows that are done stay in the batch as no-ops (they are prefilled as one pad token and fed pad): the batch is
    never compacted, so the engine and, for the Performer, its feature maps (those of the first loop: redraw off) are the same objects
    through all phases.  Token / segment rows and score tables are double-buffered (emo_acc_rebase never writes its source); self.home[j] is the
    buffer that holds row j's latest context.  The dropped tokens and their scores go to a per-row archive; results() / score_arrays() stitch
    primer + archive + context.  Phase p draws from a fresh uniform table seeded with (seed, REBASE_TAG, p).  If the one-launch step gives up,
    the phase runs again from its saved state words on the chain of launches.  self.seconds: {'rebase', 'prefill', 'capture', 'replay'} of all
    phases (capture: the run minus its replays: the graph captures and the eager steps around them)."""

    def __init__(self, loop, seed, keep=None, n_u=None, persistent=True):
        self.loop, self.model, self.dev = loop, loop.model, loop.dev
        self.W, self.temp, self.top_p, self.seed = loop.W, loop.temp, loop.top_p, int(seed)
        dev, W = self.dev, self.W
        state = loop.state.cpu().numpy()
        self.idx = [i for i in range(loop.n) if state[i, ACC_S_STATUS] == ACC_WINDOW]
        m0 = self.m0 = len(self.idx)
        assert m0 > 0, 'no stream reached the window'
        self.keep = check_rebase_keep(keep, W, max(loop.primer_lens[i] for i in self.idx), loop.longest_bar)
        # a phase steps its rows up to the window: with fewer positions than that a re-anchored row could have none left (AccompanimentQueue's refusal)
        if self.model.use_pe and self.model.pe.pe.shape[0] < W:
            raise EmoError("generate_accompaniments(window='rebase'): the positional table has %d rows, fewer than the window of %d tokens"
                           % (self.model.pe.pe.shape[0], W))
        sel = torch.tensor(self.idx, dtype=torch.long, device=dev)
        self.seq_pp = [loop.seq[sel].contiguous(), None]
        self.segs_pp = [loop.segs[sel].contiguous(), None]
        self.seq_pp[1], self.segs_pp[1] = torch.zeros_like(self.seq_pp[0]), torch.zeros_like(self.segs_pp[0])
        self.params = loop.params[sel].contiguous()
        self.state = loop.state[sel].contiguous()
        self.primer_len = torch.tensor([loop.primer_lens[i] for i in self.idx], dtype=torch.int32, device=dev)
        self.accepted0 = int(self.state[:, ACC_S_ACCEPTED].sum().item())
        cap = int(state[self.idx, ACC_S_LEN].max()) + loop.max_events + loop.longest_bar + 2       # the whole piece
        self.arch_tok = torch.zeros(m0, cap, dtype=torch.int64, device=dev)
        self.arch_len = torch.zeros(m0, dtype=torch.int32, device=dev)
        self.new_len = torch.zeros(m0, dtype=torch.int32, device=dev)
        self.running = torch.zeros(1, dtype=torch.int32, device=dev)
        self.U = torch.zeros(int(n_u or 4 * W), m0, dtype=torch.float32, device=dev)
        self.tok = torch.full((m0,), loop.pad, dtype=torch.int64, device=dev)
        self.segv = torch.ones(m0, dtype=torch.int64, device=dev)
        self.logits = torch.zeros(m0, self.model.n_token, dtype=torch.float32, device=dev)
        self.cur, self.home, self.rebased = 0, [0] * m0, [0] * m0      # (rebased[j]: the phases row j took part in)
        self.phases, self.steps, self.prefill_tokens = 0, 0, []
        self.seconds = {'rebase': 0.0, 'prefill': 0.0, 'capture': 0.0, 'replay': 0.0}
        self.bound = W
        self.persistent = persistent
        with torch.no_grad():
            self.eng = AccompanimentLoop._make_engine(self, m0, persistent, False)
        self._build_block(ops.GRAMMAR_ACC, False, loop.job_controls.take(self.idx), n_rows=m0, n_token=self.model.n_token, ld_u=m0, temperature=self.temp,
                          top_p=self.top_p, max_len=W, track_full=loop.track_full, pad=loop.pad, logits=self.logits, u_steps=self.U,
                          ev_flags=loop.ev_flags, ev_beat=loop.ev_beat, lead_tok=loop.lead_tok, lead_off=loop.lead_off, params=self.params,
                          state=self.state, seq=self.seq_pp[0], segs=self.segs_pp[0], tok_out=self.tok, seg_out=self.segv, running=self.running)
        self.scores_pp = self.arch_scores = None
        if loop.score_tables is not None:                       # the first loop's recorded draws travel with the token rows
            self.scores_pp = [{k: t[sel].contiguous() for k, t in loop.score_tables.items()}, ops.draw_score_tables(self.seq_pp[1])]
            self.arch_scores = ops.draw_score_tables(self.arch_tok)
            self.score_tables = self.scores_pp[0]

    def one_step(self):
        self.grammar()
        self.eng.step(self.tok, self.segv, dev_pos=True, logits_out=self.logits)

    _live = AccompanimentLoop._live

    def _phase_table(self):
        """The phase's uniforms, into the table the block points to."""
        gen = torch.Generator(device=self.dev)
        gen.manual_seed((self.seed * 0x9E3779B1 + REBASE_TAG * 0x85EBCA6B + self.phases) & 0x7FFFFFFFFFFFFFFF)
        self.U.copy_(torch.rand(self.U.shape, device=self.dev, generator=gen))

    def phase(self, use_graph=True, steps_per_graph=None):
        """One rebase, prefill and in-window run -> whether a row went on (False: no row was at WINDOW, or none could be re-anchored)."""
        src, dst = self.cur, 1 - self.cur
        saved = (self.state.clone(), self.params.clone(), self.arch_len.clone())
        while True:
            t0 = time.perf_counter()
            self.running.zero_()
            sc = self.scores_pp
            ops.acc_rebase(self.seq_pp[src], self.segs_pp[src], self.state, self.params, self.primer_len, self.loop.track_leadsheet,
                           self.keep, self.W, self.loop.longest_bar, self.loop.pad, self.seq_pp[dst], self.segs_pp[dst], self.arch_tok, self.arch_len,
                           self.new_len, self.running, scores=sc and sc[src], dst_scores=sc and sc[dst], arch_scores=self.arch_scores)
            nl = self.new_len.cpu().numpy()                     # (synchronises: once per phase)
            t1 = time.perf_counter()
            self.seconds['rebase'] += t1 - t0
            if int(nl.max()) == 0:
                return False
            lmax = int(nl.max())
            self.logits.copy_(self.eng.prefill(self.seq_pp[dst][:, :lmax].contiguous(), self.segs_pp[dst][:, :lmax].contiguous(),
                                               lens=self.new_len.clamp(min=1)))
            self.eng.pos_auto = True
            self._phase_table()
            ops.block_set(self._gargs, self._gheld, seq=self.seq_pp[dst], segs=self.segs_pp[dst], **(sc[dst] if sc else {}))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            self.seconds['prefill'] += t2 - t1
            try:
                pos = self._replay(lmax, self.bound, use_graph, steps_per_graph)
                if self._live() > 0:
                    self.grammar()
                torch.cuda.synchronize()
                break
            except _GaveUp as e:
                if not self.persistent:
                    raise
                print('[gen] %s -> the phase again on the chain of launches' % e)
                for t, s in zip((self.state, self.params, self.arch_len), saved):
                    t.copy_(s)
                self.persistent = False
                self.eng = AccompanimentLoop._make_engine(self, self.m0, False, False)
        t3 = time.perf_counter()
        self.seconds['replay'] += self.replayed[1]
        self.seconds['capture'] += t3 - t2 - self.replayed[1]
        self.steps += pos - lmax
        self.prefill_tokens.append(int(nl.sum()))
        for j in range(self.m0):
            if nl[j] > 0:
                self.home[j] = dst
                self.rebased[j] += 1
        self.cur = dst
        if sc:
            self.score_tables = sc[dst]
        self.phases += 1
        # a row still RUNNING stopped at the bound of the longest row: it is re-anchored with it
        status = self.state[:, ACC_S_STATUS]
        status.masked_fill_(status == ACC_RUNNING, ACC_WINDOW)
        return True

    def run(self, use_graph=True, steps_per_graph=None, max_phases=None):
        """Phases until no row is at WINDOW (or `max_phases` phases have run: benchmarks)."""
        with scoring.eval_mode(self.model), torch.no_grad():
            while max_phases is None or self.phases < max_phases:
                if not (self.state[:, ACC_S_STATUS] == ACC_WINDOW).any().item() or not self.phase(use_graph, steps_per_graph):
                    break

    def accepted_draws(self):
        return int(self.state[:, ACC_S_ACCEPTED].sum().item()) - self.accepted0

    def _stitched(self, rows_pp, archive, dtype):
        """Per stream primer + archive + context, from the buffers of rows_pp by self.home."""
        state, alen, P = self.state.cpu().numpy(), self.arch_len.cpu().numpy(), self.primer_len.cpu().numpy()
        host = [t.cpu().numpy() for t in rows_pp]
        arch = archive.cpu().numpy()
        out = []
        for j in range(self.m0):
            row, ln = host[self.home[j]][j], int(state[j, ACC_S_LEN])
            out.append(np.array(rebase_stitch(row[:P[j]], arch[j, :alen[j]], row[P[j]:ln]), dtype=dtype))
        return out

    def results(self):
        """Per WINDOW stream, in the order of self.idx, what _Stream.result() gives (or an EmoError, as AccompanimentLoop.results)."""
        status = self.state[:, ACC_S_STATUS].cpu().numpy()
        out = []
        for j, (i, ids) in enumerate(zip(self.idx, self._stitched(self.seq_pp, self.arch_tok, np.int64))):
            if status[j] == ACC_BAR_TOO_LONG:
                out.append(EmoError('generate_accompaniments: stream %d: a bar longer than the window' % i))
                continue
            out.append(_stream_result(int(status[j]), [int(t) for t in ids], 'stream %d used all %d uniforms of a rebase phase\'s table' % (i, self.U.shape[0]),
                                      'stream %d: token row, archive or lead-sheet table too short past the window' % i,
                                      'stream %d still running after %d rebase phases' % (i, self.phases)))
        return out

    def score_arrays(self, tables=None):
        """-> {'logp', 'rank', 'entropy'}: [m0, longest piece] host arrays stitched like results() (sentinels behind a piece's end)."""
        if self.scores_pp is None:
            raise EmoError('RebaseLoop.score_arrays(): the first loop was built without scores=True')
        out = {}
        for k in ('logp', 'rank', 'entropy'):
            fill, dt = (-1, np.int32) if k == 'rank' else (np.nan, np.float32)
            rows = self._stitched([t['tok_' + k] for t in self.scores_pp], self.arch_scores['tok_' + k], dt)
            a = np.full((self.m0, max(len(r) for r in rows)), fill, dtype=dt)
            for j, r in enumerate(rows):
                a[j, :len(r)] = r
            out[k] = a
        return out


def generate_accompaniments(model, event2idx, idx2event, lead_sheets, primers, max_events=10000, skip_check=False, max_bars=None, temp=1.2, top_p=0.9,
                            inadmissibles=None, seed=0, use_graph=True, best_of=1, window='host', best_by='forward', return_scores=False, slots=None,
                            banned=None, rebase_keep=None):
    """The throughput path of generate_conditional_batch: the same arguments (no per-stream samplers) and result per stream, every draw and
    the grammar of _Stream.offer on the device (emo_grammar_step), each token step = grammar launch + one engine step (the one-launch
    persistent step where the engine has one), k steps captured once as a hipGraph (EMO_GEN_GRAPH_STEPS, default 16) and replayed until
    every stream has finished.  Draws come from a uniform table [4 * max_dec_inp_len, n] seeded with `seed` (like generate_streams), so ids
    are not NumPy-RNG-identical to generate_conditional_batch; they equal the host grammar driven by the same device draws.  A stream that
    reaches the max_dec_inp_len window is finished on the host by _resume_windowed, whose draws (NumPy, seeded with (seed, i)) do not come
    from the device table (window = 'device' below finishes such streams on the device).  If the one-launch step gives up, the batch is run
    again from the start on the chain of launches, with the same table.  -> (results, seconds); a stream whose table runs out holds an
    EmoError.

    best_of = N > 1: every lead sheet runs as N streams of the same batch (stream i * N + c is candidate c of lead sheet i; each stream has its
    own column of the uniform table, so the draws differ), every finished candidate is scored (scoring.targets_of + score_tokens: mean negative
    log-probability over its Track_Full targets, on its first max_dec_inp_len tokens) and the candidate with the lowest one is returned; ties go
    to the lowest candidate index, a candidate that failed never wins.  -> (results, seconds, picks), picks[i] = {'chosen': c, 'nll_mean': [N
    floats, NaN for a failed candidate], 'candidates': [N results]}.  best_of = 1 is the path above, draw for draw.

    window = 'device': the streams that reach the window are finished together on the device by a WindowedLoop (one batched full-window
    forward and one windowed emo_grammar_step per draw, no host round trip per token) instead of one at a time by _resume_windowed.  Every id up to
    a stream's handoff is the one window = 'host' gives; past it the draws come from the windowed phase's own uniform table (seeded with (seed,
    WINDOW_TAG)), so the continuation equals the host grammar on those draws, not the NumPy draws of _resume_windowed.

    best_by = 'draws': the candidates are ranked by what the grammar launch recorded at each draw instead (scoring.draw_scores_mean: mean -logp
    over a candidate's drawn tokens; NaN for one that failed or drew nothing) and no second forward runs.  These are the probabilities of the
    generating steps themselves: under the engine's own random features, over the whole piece (with window = 'device' past the window too).
    They cover the drawn tokens the result keeps.  'forward' scores the targets of scoring.targets_of: the same tokens (everything inside a
    Track_Full span up to and including the bar's Track_LeadSheet was drawn), plus an EOS target at the end of the last span, which stands for
    the final draw that the result cuts off, and only on the first max_dec_inp_len tokens.

    return_scores = True: the result tuple gets one more element at its end, a list aligned with the results: {'logp', 'rank', 'entropy'} numpy
    arrays with one entry per id (NaN / -1 where the id was given: primer, injected bars, Track_Full; and, with window = 'host', from a
    stream's hand-off on, where _resume_windowed draws on the host), or None where the result is an error.  With best_of > 1 these are the
    chosen candidates' and every pick also carries 'scores': the N candidates'.  The ids are those of the call without it.

    slots = None: one lock-step batch with a row per stream (the paths above, draw for draw).  slots = S: the streams (lead sheets times best_of)
    are JOBS that run through S rows (AccompanimentQueue), also when S is at least their number: a row whose job ends takes the next job on the
    device, so no row idles while jobs wait and no batch waits for its longest member.  There is no prefill; a job draws from its own column of
    the uniform table, so its ids do not depend on S or on the slot it ran in beyond what the model step's arithmetic does; they are not those
    of slots = None, whose streams share a prefill.  All jobs run under the engine's one set of feature maps.  A job that reaches the window
    frees its slot and is finished after the queue has drained, by `window` as above.  Refused (EmoError) when the model's positional table has
    fewer rows than the window.  The results, best_of, best_by and return_scores are per job as they are per stream.

    window = 'rebase' (rebase_keep = None: max_dec_inp_len // 2, read at call time): a stream that fills the window drops its oldest whole bars,
    keeps its primer and goes on from a context of at most rebase_keep tokens with positions from 0 (RebaseLoop, rebase_plan): one prefill per
    phase, then the cached one-token step again, instead of a full-window forward per draw.  This is the context the reference's dataloader
    trains on (the piece's opening events followed by the piece from a bar on); it is NOT the reference's sliding window, so past a stream's
    first hand-off the ids are neither those of window = 'host' nor of 'device'.  Up to the hand-off they are.  The continuation obeys the
    same grammar, keeps the stream's ban, temp and top_p, its bar, position, failed and accepted counts and the whole-piece max_events, and
    draws from per-phase uniform tables seeded with (seed, REBASE_TAG, phase).  A stream whose last bar alone does not fit below the window
    holds an EmoError ("a bar longer than the window").  ValueError, before anything is allocated, unless len(primer) + 2 <= rebase_keep <=
    max_dec_inp_len - longest lead-sheet bar - 2, or when rebase_keep is given with another window.  best_of, best_by, return_scores, banned,
    per-stream temp / top_p and slots work as with window = 'device'.

    banned: the device form of the host loops' `inadmissibles` (which stays refused here: its one index array for all streams is not what the
    launch reads).  None: no ban; one sequence of token ids: no lead sheet's stream ever DRAWS one of them; or one entry per lead sheet, each
    a sequence of ids or None.  The grammar launch reads a banned token's logit as -inf (emo_hip.h: tok_mask), so the ids are those of the
    unbanned call on logits masked that way; primers, injected lead-sheet bars and Track_Full are fed as they are, and the recorded scores stay
    the model's own (unmasked).  tempo_ban() builds the reference's tempo constraint.  temp / top_p: one value, or one per lead sheet.  With
    best_of = N the N candidates of a lead sheet share its ban, temp and top_p; with slots = S they belong to the job.  A stream that leaves the
    device loop at the window keeps them: as `inadmissibles`, temp and top_p of _resume_windowed (window = 'host'), in the WindowedLoop's block
    (window = 'device').  ValueError, before anything is allocated, for an id outside [0, V), a ban that leaves no token, a per-input list of
    the wrong length, a temp <= 0 or a top_p outside (0, 1]."""
    if window not in ('host', 'device', 'rebase'):
        raise ValueError("window must be 'host', 'device' or 'rebase' (got %r)" % (window,))
    if rebase_keep is not None and window != 'rebase':
        raise ValueError("rebase_keep goes with window='rebase' (got window=%r)" % (window,))
    _refuse(model, inadmissibles)
    if window == 'rebase':
        rebase_keep = check_rebase_keep(rebase_keep, int(max_dec_inp_len), max([len(p) for p in primers] or [0]),
                                        max([len(b) for lead in lead_sheets for b in lead] or [0]))
        if getattr(model, 'use_pe', False) and model.pe.pe.shape[0] < int(max_dec_inp_len):       # (RebaseLoop's refusal, before the first loop runs)
            raise EmoError("generate_accompaniments(window='rebase'): the positional table has %d rows, fewer than the window of %d tokens"
                           % (model.pe.pe.shape[0], int(max_dec_inp_len)))
    best_of, by_draws, want, lead_sheets, primers = scoring.best_of_plan(best_of, best_by, return_scores, lead_sheets, primers)
    if slots is not None:
        try:
            slots = int(slots)
        except (TypeError, ValueError):
            raise ValueError('slots must be None or a count of at least 1 (got %r)' % (slots,))
        if slots < 1:
            raise ValueError('slots must be at least 1 (got %d)' % slots)
    # checked per input, before a loop allocates anything; every candidate of an input inherits the input's controls
    ctl = draw_controls('generate_accompaniments', len(lead_sheets) // best_of, model.n_token, banned, temp, top_p).repeat(best_of)
    t0 = time.time()
    kw = dict(max_events=max_events, skip_check=skip_check, max_bars=max_bars, temp=ctl.temp_arg, top_p=ctl.top_p_arg, seed=seed,
              banned=ctl.bans)

    def make(**more):
        if slots is None:
            return AccompanimentLoop(model, event2idx, idx2event, lead_sheets, primers, scores=want, **kw, **more)
        return AccompanimentQueue(model, event2idx, idx2event, lead_sheets, primers, slots, scores=want, **kw, **more)

    with scoring.eval_mode(model):
        loop = make()
        try:
            loop.run(use_graph=use_graph)
        except _GaveUp as e:
            print('[gen] %s -> the batch again on the chain of launches' % e)
            loop = make(persistent=False, redraw=False)
            loop.run(use_graph=use_graph)
        out = loop.results(event2idx, idx2event, max_events, skip_check, seed, window=window, rebase_keep=rebase_keep, use_graph=use_graph)
        sc = loop.scores(out) if want else None
        picks = None
        if best_of > 1:
            nll = scoring.draw_scores_mean(sc) if by_draws else scoring.candidate_scores(model, event2idx, out, loop.bound)
            picks = scoring.picks_of(out, nll, best_of, sc if return_scores else None)
    return scoring.generation_result(out, time.time() - t0, sc, picks, return_scores)


# ------------------------------------------------------------------------------------------------ command line (reference inference.py:330-485)
def read_lead_sheet(path, event2idx):
    """A stage-1 output file: one event per line, optionally a Key_* line first, bars opened by Bar_None.  -> (key event, [[ids of bar 0], ...])"""
    events = open(path).read().splitlines()
    key = events[0] if events and 'Key' in events[0] else 'Key_C'
    starts = [i for i, e in enumerate(events) if e == 'Bar_None'] + [len(events)]
    return key, [[event2idx[e] for e in events[a:b]] for a, b in zip(starts[:-1], starts[1:])]


def emotions_of(file_name):
    for tag, cands in (('Positive', ['Q1', 'Q4']), ('Negative', ['Q2', 'Q3']), ('Q1', ['Q1']), ('Q2', ['Q2']), ('Q3', ['Q3']), ('Q4', ['Q4']), ('None', ['None'])):
        if tag in file_name:
            return cands
    raise ValueError('wrong emotion label')


def parse_args(argv=None):
    """The command line of main(), with the refusals of flag combinations."""
    import argparse
    ap = argparse.ArgumentParser(description='stage-2 accompaniment generation on MI355X')
    req = ap.add_argument_group('required arguments')
    req.add_argument('-m', '--model_type', choices=['performer', 'gpt2'], required=True)
    req.add_argument('-c', '--configuration', required=True)
    req.add_argument('-r', '--representation', choices=['remi', 'functional'], required=True)
    ap.add_argument('-i', '--inference_params', required=True, help='checkpoint (.pt state dict)')
    ap.add_argument('-o', '--output_dir', required=True, help='directory holding the stage-1 lead sheets; results are written next to them')
    ap.add_argument('--streams', type=int, default=32, help='lead sheets generated in lock-step on one decode engine')
    ap.add_argument('--max_bars', type=int, default=128)
    ap.add_argument('--dtype', default=None, choices=[None, 'bf16', 'fp32'])
    ap.add_argument('--device', action='store_true', help='draws and grammar on the device (generate_accompaniments) instead of the host loop')
    ap.add_argument('--seed', type=int, default=0, help='--device: seed of the uniform table (the group of streams j uses seed + j)')
    ap.add_argument('--best-of', dest='best_of', type=int, default=1,
                    help='--device: candidates generated per lead sheet; the one with the lowest mean negative log-probability is written')
    ap.add_argument('--window', choices=['host', 'device', 'rebase'], default='host',
                    help='--device: streams past the %d-token window are finished one at a time on the host, together on the device, or (rebase) '
                         're-anchored on a bar and continued with cached one-token steps' % max_dec_inp_len)
    ap.add_argument('--rebase-keep', dest='rebase_keep', type=int, default=None, metavar='N',
                    help='--window rebase: the largest context a re-anchored stream starts from (default: half the window)')
    ap.add_argument('--best-by', dest='best_by', default='forward', choices=['forward', 'draws'],
                    help='--best-of: rank the candidates by a scoring forward over the finished pieces, or by the log-probabilities recorded at each draw')
    ap.add_argument('--slots', type=int, default=None,
                    help='--device: run ALL lead sheets (times --best-of) as queued jobs through this many rows of one decode engine, refilled on the device')
    ap.add_argument('--scores', default=None, metavar='FILE',
                    help='--device: write one JSON record per piece (scoring.draw_record) and its per-token logp / rank / entropy, as recorded at each draw')
    ap.add_argument('--tempo', type=int, default=None, metavar='T',
                    help='never draw a Tempo event further than --tempo-tolerance from T (tempo_ban): with --device in the grammar launch, else '
                         'as the host loop\'s inadmissibles')
    ap.add_argument('--tempo-tolerance', dest='tempo_tolerance', type=int, default=None, metavar='N', help='--tempo: the distance allowed (default 20)')
    args = ap.parse_args(argv)
    if args.tempo_tolerance is not None and (args.tempo is None or args.tempo_tolerance < 0):
        ap.error('--tempo-tolerance goes with --tempo T and is at least 0')
    if args.tempo is not None and args.tempo_tolerance is None:
        args.tempo_tolerance = 20
    if args.best_of < 1 or (args.best_of > 1 and not args.device):
        ap.error('--best-of needs --device and a count of at least 1')
    if args.window != 'host' and not args.device:
        ap.error('--window %s needs --device' % args.window)
    if args.rebase_keep is not None and args.window != 'rebase':
        ap.error('--rebase-keep goes with --window rebase')
    if args.best_by != 'forward' and args.best_of < 2:
        ap.error('--best-by goes with --best-of N, N > 1')
    if args.scores and not args.device:
        ap.error('--scores needs --device')
    if args.slots is not None and (not args.device or args.slots < 1):
        ap.error('--slots needs --device and a count of at least 1')
    return args


def main(argv=None):
    """Same flags as the reference's stage-2 inference.py (-m / -c / -r / -i / -o): every lead sheet found in the output directory gets its
    accompaniment, all jobs of a run in lock-step on ONE decode engine (--streams at a time): generate_conditional_batch (NumPy sampling and
    grammar on the host, seeds 0, 1, ... in job order), or with --device generate_accompaniments (device draws and grammar).  The generated
    events are written as text
    (`<piece>_<emotion>_full.txt`, one event per line); turning them into MIDI is the reference's convert2midi.py (needs miditoolkit) and
    is run on those files when that module is importable."""
    import yaml
    from . import train as tr
    from .data import load_vocab
    args = parse_args(argv)
    conf = yaml.load(open(args.configuration), Loader=yaml.FullLoader)
    torch.cuda.set_device(conf['training']['gpuid'])
    event2idx, idx2event, pad = load_vocab(conf['data_loader']['vocab_path'].format(args.representation))
    model = tr.build_model(args.model_type, pad + 1, conf['model'], args.dtype).cuda()
    tr.load_pretrained(model, args.inference_params)
    model.eval()
    temp, top_p = (1.1, 0.99) if args.model_type == 'performer' else (1.2, 0.97)
    print('[info] temp = %s | top_p = %s' % (temp, top_p))
    pat = 'roman.txt' if args.representation == 'functional' else '.txt'
    jobs = []
    for f in sorted(os.listdir(args.output_dir)):
        if pat not in f or f.endswith('_full.txt'):
            continue
        key, bars = read_lead_sheet(os.path.join(args.output_dir, f), event2idx)
        for e in emotions_of(f):
            out = os.path.join(args.output_dir, '_'.join(f.split('_')[:2]) + '_' + e + '_full.txt')
            if os.path.exists(out):
                print('[info] %s exists, skipping ...' % out)
                continue
            primer = [event2idx['Emotion_%s' % e]] + ([event2idx[key]] if args.representation == 'functional' else []) + [event2idx['Tempo_110']]
            jobs.append((out, key, bars, primer))
    print('[# jobs]', len(jobs))
    ban = tempo_ban(event2idx, args.tempo, args.tempo_tolerance) if args.tempo is not None else None
    if ban is not None:
        print('[info] tempo %d +- %d: %d tempo events banned' % (args.tempo, args.tempo_tolerance, len(ban)))
    per_group = max(1, args.streams // args.best_of)              # --streams counts engine streams: N of them per lead sheet with --best-of N
    if args.slots is not None:
        per_group = max(1, len(jobs))                             # one call: the jobs queue for the slots
    want, score_pieces = bool(args.scores), []
    for j, i in enumerate(range(0, len(jobs), per_group)):
        group = jobs[i:i + per_group]
        if args.device and args.best_of > 1:
            gen, _, picks, *sc = generate_accompaniments(model, event2idx, idx2event, [g[2] for g in group], [g[3] for g in group],
                                                         max_bars=args.max_bars, temp=temp, top_p=top_p, seed=args.seed + j, best_of=args.best_of,
                                                         window=args.window, best_by=args.best_by, return_scores=want, slots=args.slots,
                                                         banned=ban, rebase_keep=args.rebase_keep)
            for g, p in zip(group, picks):
                print('[info] %s: candidate %d of %s' % (g[0], p['chosen'], ['%.4f' % x for x in p['nll_mean']]))
        elif args.device:
            gen, _, *sc = generate_accompaniments(model, event2idx, idx2event, [g[2] for g in group], [g[3] for g in group], max_bars=args.max_bars,
                                                  temp=temp, top_p=top_p, seed=args.seed + j, window=args.window, return_scores=want, slots=args.slots,
                                                  banned=ban, rebase_keep=args.rebase_keep)
        else:
            gen = generate_conditional_batch(model, event2idx, idx2event, [g[2] for g in group], [g[3] for g in group], max_bars=args.max_bars,
                                             temp=temp, top_p=top_p, seeds=list(range(i, i + len(group))),
                                             inadmissibles=np.array(ban, np.int64) if ban else None)
        if want:
            score_pieces += scoring.draw_pieces([os.path.basename(g[0]) for g in group], gen, sc[0])
        for (out, key, _, _), ids in zip(group, gen):
            if isinstance(ids, Exception):
                print('[info] %s not written: %s' % (out, ids))
                continue
            with open(out, 'w') as fh:
                fh.write('\n'.join([key] + [idx2event[w] for w in ids]) + '\n')
            print('[info] wrote', out, len(ids), 'events')
    if want:
        scoring.write_draw_scores(args.scores, score_pieces)
        print('[info] wrote', args.scores, len(score_pieces), 'records')
    try:
        import convert2midi  # noqa: F401  (the reference's module, if the user put it on the path together with miditoolkit)
        print('[info] convert2midi is importable: run it on the *_full.txt files to obtain MIDI')
    except ImportError:
        print('[info] event files written; MIDI conversion (reference convert2midi.py, needs miditoolkit) is outside this package')


if __name__ == '__main__':
    main()
