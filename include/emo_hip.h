/*
 * emo_hip.h — C-ABI of libemo_hip.so: the MI355X (gfx950) kernels behind the
 * stage-2 causal-LM hot path of EMO-Disentanger (Performer / GPT-2 backbones).
 *
 * The reference has NO FFI: its seam is the Python object contract of
 * MusicPerformer / MusicGPT2.  Each entry point below cites
 * the reference lines (relative to /root/reference/stage2_accompaniment) whose
 * arithmetic it replaces; the Python classes in emo-disentanger_amd/model/
 * bind them through ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller (torch tensors);
 *     the library never allocates or frees tensor memory; scratch is caller-provided
 *     after the matching *_workspace_bytes() query;
 *   - every launch takes an explicit hipStream_t (as void*) and is asynchronous;
 *   - return value: 0 = ok, <0 = error (emo_last_error() gives a thread-local message);
 *   - dims are int64_t, row-major; "ld" = row stride in ELEMENTS;
 *   - dtype: EMO_F32 (parity mode: exact-f32 MFMA/VALU math) or EMO_BF16 (speed mode:
 *     bf16 storage + bf16 MFMA, fp32 accumulation / statistics / scan state).
 *   - dropout masks are never stored: forward and backward regenerate them from
 *     (seed, offset, linear element index).
 */
#ifndef EMO_HIP_H
#define EMO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* emo_stream_t; /* hipStream_t */

enum { EMO_OK = 0, EMO_ERR_INVALID = -1, EMO_ERR_LAUNCH = -2, EMO_ERR_UNSUPPORTED = -3 };
enum { EMO_F32 = 0, EMO_BF16 = 1, EMO_I64 = 2 /* emo_comm_* payloads only */ };
enum { EMO_ACT_NONE = 0, EMO_ACT_RELU = 1, EMO_ACT_GELU_NEW = 2, EMO_ACT_GELU = 3 };   /* GELU_NEW: HF tanh form (GPT-2); GELU: exact erf form
                                                                                       * (F.gelu: the Performer stack's activation='gelu', fast_transformer_decoder.py:50) */
enum { EMO_MUL_NONE = 0, EMO_MUL_NONZERO = 1, EMO_MUL_DGELU_NEW = 2, EMO_MUL_BITMASK = 3, EMO_MUL_DGELU = 4 };   /* DGELU: *= d/dx of the erf form at mul_aux */

int emo_version(void);
/* build options of the library: bit 0 = the opt-in experimental GEMM kernels (emo_gemm_p256.hip: persistent 256 x 256 tile walk, 128 x 512 tile — measured
 * negatives inside the training step, built only with `make EXTRA=-DEMO_EXPERIMENTAL`; without them EMO_GEMM_P256 / EMO_GEMM_Q512 have no effect) */
int emo_build_flags(void);
const char* emo_last_error(void);
/* number of CUs of the current device (for grid sizing on the host side) */
int emo_device_cus(void);

/* ------------------------------------------------------------------ K2/K7/K8: dense GEMM on MFMA
 * C[M,N] = epilogue( A·B )   with
 *   a_trans=0: A stored [M,K] (k contiguous)      a_trans=1: A stored [K,M]
 *   b_trans=0: B stored [N,K] (nn.Linear weight)  b_trans=1: B stored [K,N] (HF Conv1D weight)
 * epilogue order: +bias[n] -> (aux_out = value) -> act -> *mul(mul_aux) -> dropout -> +residual
 * Replaces: F.linear in fast-transformers AttentionLayer / TransformerEncoderLayer
 * (called from model/fast_transformer_decoder.py:28-51), HF Conv1D addmm in GPT2Attention /
 * GPT2MLP (model/music_gpt2.py:42-51,86), dec_out_proj (music_performer.py:27,65), and their
 * autograd backward (dgrad / wgrad).
 */
typedef struct {
    const float* bias;    /* [N] fp32 or NULL */
    int act;              /* EMO_ACT_* */
    void* aux_out;        /* NULL or [M,N] (dtype_out, ld=ldc): value before the activation */
    const void* mul_aux;  /* NULL or [M,N] (dtype_out, ld=ldc), see mul_mode */
    int mul_mode;         /* EMO_MUL_NONZERO: *= (mul_aux!=0)*mul_scale ; EMO_MUL_DGELU_NEW: *= gelu_new'(mul_aux) ;
                           * EMO_MUL_BITMASK: mul_aux is the uint8 bit mask (M*N/8 bytes, tiled layout) written by mask_out, *= bit ? mul_scale : 0 */
    float mul_scale;
    float p_drop;         /* dropout after the activation; element index = m*N+n */
    uint64_t seed, offset;
    const void* residual; /* NULL or [M,N] (dtype_out, ld=ldc) added last */
    /* LayerNorm folded around a decode-step GEMM (bf16, M <= 32, NT; any other shape is refused).  With A' = LN(A)*gamma + beta:
     *   A'.W^T [m][n] = rstd[m] * ((A.(gamma*W)^T)[m][n] - mean[m]*c1[n]) + (beta.W^T)[n],   c1[n] = sum_k gamma[k] W[n][k]
     * the caller passes B = gamma*W, ln_c1 = c1 and folds beta.W^T into `bias`; mean/rstd of the A rows are computed in-kernel
     * (biased variance, ln_eps inside the sqrt: nn.LayerNorm) and optionally exported.  rln_*: the residual is LayerNorm(rln_x)
     * rebuilt from exported statistics (added before bias; needs act = none, no dropout).  Replaces the standalone norm1 / norm2
     * launches of fast-transformers' TransformerEncoderLayer on the one-token decode path. */
    const float* ln_c1;       /* NULL or [N] */
    float ln_eps;
    float* ln_stats_out;      /* NULL or [M,2] (mean, rstd) of the A rows */
    const void* rln_x;        /* NULL or [M,N] (dtype_out, ld=ldc): raw tensor whose LayerNorm is the residual */
    const float* rln_stats;   /* [M,2] (mean, rstd) of the rln_x rows */
    const float* rln_gamma;   /* [N] */
    const float* rln_beta;    /* [N] */
    float* a_rowsum;      /* NULL or [M] fp32: += sum_k op(A)[m][k]; needs a_trans.  For a weight gradient dW = dY^T X this is the bias
                           * gradient (column sums of dY), taken inside the GEMM from the operand fragments instead of a second pass. */
    float* b_rowsum;      /* NULL or [N] fp32: += sum_k op(B)[n][k]; needs a_trans and b_trans (HF Conv1D layout, where dY is the B operand) */
    uint8_t* mask_out;    /* NULL or M*N/8 bytes: one bit per output = (value after act and dropout != 0) — the 1-bit relu.dropout mask the FFN2
                           * dgrad needs (instead of re-reading the [M,N] activation).  TILED layout (r03, byte order r05; only emo_gemm reads it back): the 256
                           * bytes of a 32-row x 64-column tile are contiguous at ((m/32)*(N/64) + n/64)*256; inside, byte
                           * ((n%32)/8*16 + m%16)*4 + (m%32)/16*2 + (n%64)/32 holds columns 8*(n/8) .. +7 of row m, bit j = column 8*(n/8)+j
                           * (a lane's four bytes of a tile are one dword: ONE 256-byte store / load per wave of the A-stationary kernel).  Only with EMO_MUL_BITMASK's
                           * shape class: bf16 in/out, NT, K = 512, M % 128 == 0, M >= 4096, N % 64 == 0, N <= 2048 (the A-stationary kernel); refused elsewhere. */
    void* workspace;      /* NULL or caller scratch for split-K partial sums (plain fp32-output GEMMs = weight gradients): */
    int64_t workspace_bytes; /* with it the splits are summed in a fixed order by a reduce kernel (deterministic, no atomics);
                              * without it they are fp32 atomics into C.  Size: emo_gemm_workspace_bytes(). */
    /* LayerNorm of the A operand inside the product (r05; replaces the standalone norm launch in front of a Linear — norm1 -> linear1 of
     * fast-transformers' TransformerEncoderLayer via fast_transformer_decoder.py:45-51, ln_1 -> c_attn / ln_2 -> c_fc of HF GPT2Block via
     * music_gpt2.py:42-51): A is the RAW tensor; the A-stationary kernel, which holds complete 512-wide rows in registers, computes
     * mean / rstd per row (biased variance, ln_eps inside the sqrt), normalises in place with lna_gamma / lna_beta [K] and, besides the product,
     * writes the normalised rows to lna_out [M, K] (dtype_in, contiguous: residual of the next Linear, operand of the weight gradient) and the
     * statistics to lna_mean / lna_rstd [M].  Only in the A-stationary shape class (bf16, NT, K = 512, M % 128 == 0, M >= 4096); refused elsewhere. */
    const float* lna_gamma;
    const float* lna_beta;
    void* lna_out;
    float* lna_mean;
    float* lna_rstd;
    /* Per-row, per-64-column-block divisor (r06): C[m][n] /= hdiv[((m / hdiv_T) * (N / 64) + n / 64) * hdiv_T + m % hdiv_T] — with hdiv = the FAVOR+
     * normaliser den [B, H, T] (emo_attn_t.den) and C = d(attention output) = the out-projection's dgrad, the product leaves as dN = dout / den
     * (the first thing both backward sweeps of causal_product form), in ONE rounding from the fp32 accumulators, and
     * the FAVOR backward takes it without the normaliser (emo_attn_t.dout_is_dn).  Replaces the d(out)/den scalings inside the causal_product backward reached from
     * fast_transformer_decoder.py:33-40.  Only with a plain epilogue in the A-stationary class (bf16 in / out, NT, K = 512, M % 128 == 0, M >= 4096,
     * N % 64 == 0) and hdiv_T % 32 == 0, M % hdiv_T == 0; refused elsewhere. */
    const float* hdiv;
    int64_t hdiv_T;
} emo_epilogue_t;

/* scratch that lets emo_gemm() run its split-K without atomics (0 = this problem is not split) */
/* diagnostics: kernel family of the calling thread's last emo_gemm (1 skinny, 2 A-stationary K = 512, 3 / 4 256 x 256 tile wgrad / NT,
 * 5 / 6 128 x 128 LDS-DMA / register-staged, 7 exact-fp32, 8 persistent 256 x 256 tile walk (EMO_GEMM_P256=1), 9 128 x 512 tile (EMO_GEMM_Q512=1); + 16 split-K via the workspace, + 32 with the reduce-and-epilogue pass) */
int emo_gemm_last_kernel(void);
/* diagnostics: what ran inside that family, for the calling thread's last emo_gemm:
 *   BK | stages << 8 | splits << 16 | astat_column_split << 24        (a zero field = the family has none)
 * BK: depth of one K step (LDS-DMA ring 32 / 64, register-staged 64, fp32 16, A-stationary 128, 256 x 256 tiles 64; skinny: the 64- / 128-wide chunk);
 * stages: slots of the ring (skinny: waves per block; register-staged and fp32: 0);  splits: K-splits that ran (0 = unsplit; the 256 x 256 wgrad kernel's
 * full + extra splits);  astat_column_split: blocks that share a 128-row panel of the A-stationary kernel (1 = one block sweeps all of N). */
int emo_gemm_last_plan(void);
/* sizeof(emo_epilogue_t) as the library was built — a binding checks its own mirror of the struct against it before the first call */
int emo_epilogue_size(void);
int64_t emo_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype_in, int dtype_out);

int emo_gemm(const void* A, int a_trans, int64_t lda, const void* B, int b_trans, int64_t ldb,
             void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
             int dtype_in, int dtype_out, int accumulate /* C += result; fp32 out only */,
             const emo_epilogue_t* epi /* may be NULL */, emo_stream_t stream);
/* The route emo_gemm would take for these arguments, without launching anything: EMO_OK and the two words emo_gemm_last_kernel() /
 * emo_gemm_last_plan() would show after that call (either pointer may be NULL), or the error emo_gemm would return.  Operand pointers are used for
 * their alignment only; the calling thread's last-kernel / last-plan words are left alone.  Needs no GPU. */
int emo_gemm_route(const void* A, int a_trans, int64_t lda, const void* B, int b_trans, int64_t ldb,
                   void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                   int dtype_in, int dtype_out, int accumulate, const emo_epilogue_t* epi, int* kernel, int* plan);
/* 1 when the problem is in the class of the A-stationary K = 512 kernel as far as that does not depend on the tensors (shape, dtypes, switches: the
 * predicate the planner itself uses) — the class in which mask_out / EMO_MUL_BITMASK / lna_* / hdiv exist.  emo_gemm_astat_min_rows(): the fewest rows
 * of that class (4096; EMO_ASTAT_MIN_ROWS). */
int emo_gemm_astat_supported(int dtype_in, int dtype_out, int64_t M, int64_t N, int64_t K);
int64_t emo_gemm_astat_min_rows(void);

/* ------------------------------------------------------------------ K7f: the feed-forward block in one launch (r06)
 *   h1 = LayerNorm(x1) * gamma + beta;  f = dropout(relu(h1 W1^T + b1));  x2 = h1 + dropout(f W2^T + b2)
 * Replaces `norm1 -> linear1 -> activation -> dropout -> linear2 -> dropout -> + residual` of fast-transformers' TransformerEncoderLayer.forward
 * as called from model/fast_transformer_decoder.py:45-51 (two emo_gemm launches until r05).  W1 [d_ff, d_model], W2 [d_model, d_ff] are the
 * nn.Linear weights (bf16 mirrors, k-contiguous rows), b1 / b2 fp32.  Outputs: h1_out [M, d_model] (the residual; operand of the FFN1 weight gradient),
 * mean_out / rstd_out [M] (LayerNorm backward), f_out [M, d_ff] (operand of the FFN2 weight gradient), mask_out (M * d_ff / 8 bytes: the 1-bit
 * relu.dropout mask in emo_epilogue_t.mask_out's tiled layout, read back by EMO_MUL_BITMASK in the FFN2 dgrad), x2_out [M, d_model].  The hidden
 * activation is written once and never re-read in the forward; the residual never leaves the registers.  Dropout element indices as in emo_gemm:
 * (seed, offset_f, m * d_ff + n) for f and (seed, offset_y, m * d_model + n) for the FFN2 output — results are bit-identical to the two-launch
 * form.  Served for bf16, d_model 512, d_ff 2048, M % 128 == 0, M >= 32768 (emo_ffn_fwd_supported() = 1); EMO_ERR_INVALID elsewhere. */
int emo_ffn_fwd_supported(int dtype, int64_t M, int64_t d_model, int64_t d_ff);
int emo_ffn_fwd(const void* x1, const float* gamma, const float* beta, float ln_eps, const void* W1,
                const float* b1, const void* W2, const float* b2, void* h1_out, float* mean_out,
                float* rstd_out, void* f_out, uint8_t* mask_out, void* x2_out, int64_t M, int64_t d_model,
                int64_t d_ff, int dtype, float p_drop, uint64_t seed, uint64_t offset_f, uint64_t offset_y,
                emo_stream_t stream);

/* out[n] (+)= sum_m X[m,n] — bias gradients */
int emo_colsum(const void* X, int dtype, int64_t M, int64_t N, int64_t ld, float* out,
               int accumulate, emo_stream_t stream);

/* ------------------------------------------------------------------ K1: embedding prologue
 * out[b,t,:] = dropout( (E[tok[b,t]] + S[seg[b,t]]) * scale + pe[pos0 + pos_ids[b] + t] )   (pos_ids NULL = zeros)
 * Replaces TokenEmbedding.forward x2 + PositionalEncoding + emb_dropout
 * (model/transformer_helpers.py:81-87,57-63; model/music_performer.py:51-62).
 * pe: fp32 rows of length D (the `pe.pe` buffer [max_pos,1,D] is exactly that).
 * pos_ids (nullable, device int64 [B]): per-sequence position of its first token, replacing pos0 —
 * decode streams of different lengths, and hipGraph replay (no host-side position baked in). */
int emo_embed_fwd(const int64_t* tok, const int64_t* seg, const float* E, const float* S,
                  const float* pe, void* out, int dtype, int64_t B, int64_t T, int64_t D,
                  int64_t V, int64_t n_seg, int64_t pos0, const int64_t* pos_ids, float scale,
                  float p_drop, uint64_t seed, uint64_t offset, emo_stream_t stream);
/* dE[tok] += dout*mask*scale ; dS[seg] += ...  (fp32 accumulate, caller zeroes) */
int emo_embed_bwd(const int64_t* tok, const int64_t* seg, const void* dout, int dtype, float* dE,
                  float* dS, int64_t B, int64_t T, int64_t D, int64_t V, int64_t n_seg,
                  float scale, float p_drop, uint64_t seed, uint64_t offset, emo_stream_t stream);

/* ------------------------------------------------------------------ K6: LayerNorm (eps inside sqrt, biased var)
 * Replaces nn.LayerNorm norm1/norm2 (fast-transformers TransformerEncoderLayer) and ln_1/ln_2 (HF GPT2Block). */
int emo_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                      float* rstd, int dtype, int64_t M, int64_t D, float eps, emo_stream_t stream);
/* dx = LN'(dy) (+ dres);  dx_drop (optional) = dx * dropmask(p,seed,offset);  dgamma/dbeta += (atomic);
 * dcol (optional, fp32 [D]) += column sums of dx_drop (of dx when dx_drop is NULL) — the bias gradient of the Linear
 * whose output fed this LayerNorm's residual branch, fused here to save one pass over the tensor.
 * workspace: a caller-owned scratch for the three column sums (dgamma, dbeta, dcol): every block writes its partial sums to the workspace
 * and a second small kernel adds them in block order — no atomics, so these gradients are bit-reproducible and the 3 x D atomics per block
 * (a third of the kernel's time at 8192 rows) are gone.  emo_layernorm_bwd_workspace_bytes() = 0 means the shape takes the generic
 * kernel (atomics); workspace = NULL or too small falls back to the atomic accumulation as well.  Contents need not survive the call. */
int64_t emo_layernorm_bwd_workspace_bytes(int dtype, int64_t M, int64_t D);
int emo_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                      const float* rstd, const void* dres, void* dx, void* dx_drop, float* dgamma,
                      float* dbeta, float* dcol, int dtype, int64_t M, int64_t D, float p_drop,
                      uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes,
                      emo_stream_t stream);
/* out = x * dropmask  (backward of a dropout whose forward was fused in a GEMM epilogue) */
int emo_dropout_apply(const void* x, void* out, int dtype, int64_t n, float p_drop, uint64_t seed,
                      uint64_t offset, emo_stream_t stream);

/* ------------------------------------------------------------------ K3+K4, K5, K5r: the attention kernels of the training step and of the chain-of-launches token step
 * ONE entry, emo_attn, with ONE argument block, emo_attn_t: `kind` selects the attention, `pass` the forward, a backward pass or the one-token
 * DECODE pass of it.  q, k, v: [B*T, H*dh] views with row stride ld (a fused [B*T, 3*H*dh] projection works; batch-major); out [B*T, H*dh] (ld_out).
 * DECODE (every kind): one query row per stream, T = 1 and B = the number of streams; q, k, v are the new token's rows [B, H*dh] (read element-wise:
 * no alignment or stride rule beyond one shared ld).
 *
 * EMO_ATTN_FAVOR — FAVOR+ causal linear attention (K3+K4).  omega [dh, n_feat/2] fp32; den [B,H,T] fp32 (saved for backward).
 * state_S [B,H,n_feat,dh] / state_z [B,H,n_feat] fp32: optional final scan state (decode prefill).
 * Replaces fast-transformers Favor.forward + CausalLinearAttention.forward + native
 * causal_product (called via model/fast_transformer_decoder.py:28-40) and their backward.
 *   workspace: when B*H workgroups cannot fill the GPU (the reference's default batch_size 4 x 8 heads
 *   = 32), the scan is cut into P time segments that run in parallel: a state-only pass writes each
 *   segment's state increment to the workspace and the main pass starts every segment from the sum
 *   of the increments before it (behind it, for the reverse sweep of dk/dv).  The caller owns the
 *   scratch: emo_favor_attn_workspace_bytes() gives its size (0 = single segment; same value for
 *   fwd and bwd, contents need not survive between calls).  workspace = NULL forces P = 1.
 *   kstate_valid (BWD): when the segment-parallel scan is in use (emo_favor_attn_workspace_bytes() > 0) the backward first recomputes the per-segment
 *   K-state increments that the forward call left in ITS workspace.  A caller that kept that buffer untouched for the matching backward passes
 *   it here with kstate_valid = 1 and saves the state-only pass (one launch per layer); the buffer is then reused for the R-state increments as usual.
 *   dout_is_dn (BWD, r06): the incoming gradient is already divided by the normaliser: `dout` = dN = dout / den, as the out-projection's dgrad leaves
 *   it when its epilogue carries emo_epilogue_t.hdiv = den (one rounding from the fp32 accumulators instead of bf16(dout) then bf16(dout / den)); the
 *   kernels then need neither den nor the rescaled operand copies (dD_t = -(dN_t . out_t)), and no workspace.  Same reference lines (the native
 *   causal_product backward reached from fast_transformer_decoder.py:33-40).  Served by the single-segment slice kernels only — bf16, d_head 64,
 *   128 features, T % 32 == 0, B * H >= 256 (emo_favor_attn_bwd_dn_supported() = 1); refused elsewhere, the caller then keeps the plain form.
 *   DECODE: one recurrent step per stream on state_S / state_z (both required, read and written): state += phi(k) (x) v ;
 *   out = phi(q)^T S / (phi(q).z + eps).  16 <= dh <= 64 dividing 256, n_feat <= 128.
 *
 * EMO_ATTN_SOFTMAX — causal softmax attention (K5, GPT-2).  Replaces HF GPT2Attention._attn (model/music_gpt2.py:86):
 * softmax(q k^T/sqrt(dh) + causal) [dropout] v.  lse [B,H,T] fp32 saved for backward.  Dropout index = ((b*H+h)*T + i)*T + j.
 *   delta_ws (BWD): caller scratch [B,H,T] fp32 (dO.O per query row: written by the dQ pass, read by the dK/dV pass).
 *   keep: the attention-dropout keep decisions handed from the forward to the backward: the forward writes one bit per score at or below the
 *   diagonal (32-bit words [B*H][T/64 key tiles][2][T rows], emo_softmax_attn_keep_bytes() bytes — 0 when the call is not served by the 32 x 32
 *   MFMA kernels: then pass keep = NULL), the dK/dV pass reads the bits instead of re-evaluating the keyed hash per score.  Results are
 *   bit-identical to the calls without the buffer (same hash, evaluated once).
 *   DECODE (K5 decode): one query row per stream (the HF `past_key_values` path of GPT2Attention, model/music_gpt2.py:86) against a KV cache;
 *   lens[s] + lens_off = valid keys INCLUDING the new token.  k, v (both or neither NULL): the new token's key / value rows, appended to the caches
 *   at position len-1 by the kernel itself (the HF `past_key_values` concat of GPT2Attention).  Cache layout (r06): head_major = 0:
 *   [B, T_max, H*dh]; head_major = 1: [B, H, T_max, dh] — the keys / values of one (stream, head) are one contiguous run, which is what the one
 *   workgroup per (stream, head) streams (the layout HF's `past_key_values` itself uses: [batch, head, seq, head_dim]).  No dropout, no window.
 *
 * EMO_ATTN_RELPOS — relative-position causal attention (K5r, stage-1 Transformer-XL).  SURVEY §8 f-1.  Replaces
 * RelPartialLearnableMultiHeadAttn's score / softmax / value product (stage1_compose/model/optimus_txl_decoder.py:331-366) including
 * `_rel_shift` (:280-293):
 *   score[i][j] = ((q_i + r_w_bias).k_j + (q_i + r_r_bias).R[i-j]) / sqrt(dh),  j <= i
 *   prob = softmax -> dropout -> p / (sum_j p + 1e-8);  out = prob v
 * r_dist [n_dist >= T, H*dh] (ld_r) = r_net(pos_emb) indexed BY DISTANCE (row d = the reference's r_head_k[klen-1-d]).  r_w_bias / r_r_bias
 * [H, dh] fp32.  lse [B,H,T], zden [B,H,T] (may be NULL in FWD: the renormalisation denominator E/l + 1e-8) are saved for the backward passes.
 *   window (FWD): 0 = every key j <= i.  W > 0 = the sliding window of the one-token steps (the DECODE pass with the same window, mem_len = W
 *   of emo_decode_step's form 2): score[i][j] for max(0, i - W) <= j <= i only, same score, softmax, zden and lse over those keys — what T decode steps
 *   over a K/V cache compute, in one pass and O(T W) work (key tiles outside the band are never loaded).  r_dist then needs rows
 *   0 .. min(T - 1, W) only.  An evaluation feature: refused with p_drop > 0, and on every other kind or pass but DECODE (the backward passes are not windowed).
 *   BWD, the query-tile pass: recomputes the probabilities per query tile and returns dq = dq_content + dq_relative (dq_content = ds.K/sqrt(dh),
 *   dq_relative[i] = sum_j ds_ij R[i-j]/sqrt(dh), both accumulated in-kernel) plus dq_rel = the relative part alone ([B*T, H*dh], pitch ld_rel,
 *   dtype of q): d r_r_bias = colsum(dq_rel), d r_w_bias = colsum(dq) - colsum(dq_rel).  delta (may be NULL) [B,H,T] fp32: dO.O per query row,
 *   for the two passes below.
 *   BWD_KV, the key-tile pass: dk, dv in one kernel.  qu = q + r_w_bias, qv = q + r_r_bias [B*T, H*dh] (pitch ld_q) materialised by the
 *   caller (emo_add_bias2); delta as exported by BWD.
 *   BWD_R, the distance-window pass: dR [T, ld_dr] fp32 (overwritten) = gradient of r_dist rows 0..T-1,
 *   dR[dist][h*dh + d] = sum_{b,i} ds[b,h,i,i-dist] (q_i + r_r_bias)[d] / sqrt(dh).  One workgroup per (b, h, tile diagonal); the partial windows
 *   go through `workspace` (emo_relpos_attn_bwd_r_workspace_bytes) and are summed in a fixed order (deterministic).  qu, qv, delta as for BWD_KV.
 *   Replaces the reference's autograd through _rel_shift (optimus_txl_decoder.py:280-293, 331-366).
 *   DECODE (K5r decode): one query row per stream against a KV cache [B, T_max, H*dh] (the reference re-projects its cached hidden states `mems`
 *   every step, plain_transformer.py:52-59; k / v of a position do not change, so they are cached instead).  Keys j in [max(0, len-1-window), len)
 *   with len = lens[s] + lens_off and window = 0 for every cached key; the distance of key j is len-1-j, so r_dist needs n_dist >= T_max rows.
 *   k, v as in the SOFTMAX DECODE pass.  Eval semantics (no dropout).
 *
 * A field that a kind/pass does not read is ignored, whatever it holds (the comment of each field names its readers).  The block is read at
 * call time and holds raw device addresses: its owner keeps the memory alive until the launches are queued. */
enum { EMO_ATTN_FAVOR = 0, EMO_ATTN_SOFTMAX = 1, EMO_ATTN_RELPOS = 2 };
enum { EMO_ATTN_FWD = 0, EMO_ATTN_BWD = 1, EMO_ATTN_BWD_KV = 2 /* RELPOS */, EMO_ATTN_BWD_R = 3 /* RELPOS */, EMO_ATTN_DECODE = 4 };
typedef struct {
    int32_t kind;              /* EMO_ATTN_FAVOR / SOFTMAX / RELPOS */
    int32_t pass;              /* EMO_ATTN_FWD / BWD / DECODE; RELPOS also BWD_KV, BWD_R */
    /* --- all kinds */
    const void *q, *k, *v;     /* 16-B aligned; q: not RELPOS BWD_KV / BWD_R (they take qu, qv).  DECODE: any alignment; SOFTMAX, RELPOS: k, v both or both NULL */
    int64_t ld;                /* row stride of q, k, v: a multiple of 16 B (DECODE: any) */
    void* out;                 /* FWD, DECODE: written; BWD (all kinds): read.  16-B aligned (DECODE: any alignment) */
    const void* dout;          /* every backward pass: [B*T, H*dh] (ld_out), 16-B aligned */
    int64_t ld_out;            /* row stride of out and dout */
    void *dq, *dk, *dv;        /* BWD of FAVOR, SOFTMAX: all three; RELPOS BWD: dq, RELPOS BWD_KV: dk, dv.  16-B aligned */
    int64_t ld_d;              /* row stride of dq, dk, dv: a multiple of 4 */
    int32_t dtype;             /* EMO_F32 / EMO_BF16 of q, k, v, out and the gradients */
    int64_t B, T, H, dh;       /* DECODE: B streams, T = 1 */
    float p_drop;              /* SOFTMAX, RELPOS: dropout on the probabilities, regenerated in every pass from (seed, offset) */
    uint64_t seed, offset;
    void* workspace;           /* FAVOR (not with dout_is_dn): segment states or NULL; RELPOS BWD_R: the partial windows.  16-B aligned */
    int64_t workspace_bytes;
    /* --- FAVOR */
    const float* omega;
    float* den;                /* FWD: written; BWD: read (not with dout_is_dn) */
    float *state_S, *state_z;  /* FWD: NULL or both, written; DECODE: both, read and written */
    int64_t n_feat;            /* even; DECODE: <= 128 */
    float eps;                 /* the normaliser's epsilon */
    int32_t kstate_valid;      /* BWD: `workspace` still holds the forward's K-state increments */
    int32_t dout_is_dn;        /* BWD: dout is dN = dout / den */
    /* --- SOFTMAX, RELPOS */
    float* lse;                /* FWD: written; every backward pass: read */
    /* --- SOFTMAX */
    float* delta_ws;           /* BWD */
    void* keep;                /* NULL or the keep words: FWD writes, BWD reads */
    int64_t keep_bytes;
    /* --- RELPOS */
    const void* r_dist;        /* 16-B aligned */
    int64_t ld_r, n_dist;      /* ld_r: a multiple of 16 B; n_dist >= T (FWD with window = W > 0: >= min(T, W + 1); DECODE: >= T_max) */
    const float *r_w_bias, *r_r_bias;   /* FWD, BWD, DECODE */
    float* zden;               /* FWD: written (or NULL); every backward pass: read */
    void* dq_rel;              /* BWD.  16-B aligned */
    int64_t ld_rel;            /* BWD: a multiple of 4 */
    float* delta;              /* BWD: written (or NULL); BWD_KV, BWD_R: read */
    const void *qu, *qv;       /* BWD_KV, BWD_R.  16-B aligned */
    int64_t ld_q;              /* row stride of qu, qv */
    float* dR;                 /* BWD_R */
    int64_t ld_dr;             /* BWD_R: >= H * dh */
    int64_t window;            /* RELPOS FWD, DECODE: 0 or the band width W (keys i - W .. i; DECODE: len-1-W .. len-1); must be 0 everywhere else */
    /* --- DECODE of SOFTMAX, RELPOS */
    void *kcache, *vcache;     /* the K / V caches, read and (with k, v) appended to.  16-B aligned, H*dh a multiple of 16 B */
    int64_t T_max;             /* rows per stream (head_major: per (stream, head)) of the caches; T_max * 4 bytes of scores must fit 128 KB of LDS */
    const int64_t* lens;       /* int64 [B] on the device: lens[s] + lens_off = the valid keys of stream s, the new token included.  DECODE requires
                                * 1 <= lens[s] + lens_off <= T_max for every stream: both cache kernels index row len-1 unconditionally (they read it, and
                                * with k, v write it) and the values live on the device, where the entry cannot check them */
    int64_t lens_off;
    int32_t head_major;        /* SOFTMAX DECODE: the caches are [B, H, T_max, dh] instead of [B, T_max, H*dh] */
} emo_attn_t;
/* sizeof(emo_attn_t) as the library was built (a binding checks its mirror against it, as with emo_epilogue_size) */
int emo_attn_size(void);
/* Messages name the kind and the pass: "emo_attn[favor, fwd]: ", "emo_attn[favor, bwd, dn]: " (dout_is_dn), "emo_attn[relpos, bwd_kv]: ", "emo_attn[softmax, decode]: " ... */
int emo_attn(const emo_attn_t* args, emo_stream_t stream);
/* the sizes and classes named above: pure functions of the problem (and of the EMO_FAVOR_* switches) */
int64_t emo_favor_attn_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t dh, int64_t n_feat);
int emo_favor_attn_bwd_dn_supported(int dtype, int64_t B, int64_t T, int64_t H, int64_t dh, int64_t n_feat);
int64_t emo_softmax_attn_keep_bytes(int dtype, int64_t B, int64_t T, int64_t H, int64_t dh, float p_drop);
int64_t emo_relpos_attn_bwd_r_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t dh);
/* ONE-LAUNCH decode step: one token of every stream through a whole model in a single persistent kernel (csrc/emo_decode_persist.hip), for
 * n_streams <= 32 streams (a multiple of 4), bf16 weights: 8 groups x 32 workgroups of 12 waves (4 poller + 2 x 4 compute), a group owns 4 streams and
 * exchanges the activations of the 5 dependent products of a layer through tagged 8-byte granules.  Built for d_model 512 / 8 heads / d_ff 2048,
 * n_layers <= 15, n_token <= 512.  One argument block, emo_decode_step_t, selects the model (`form`) and whether the launch draws its own token (`sampled`):
 *   form 0, Performer: the token loop of stage2_accompaniment/inference.py:250-277 -> MusicPerformer.forward(keep_last_only), music_performer.py:50-70:
 *     embedding (transformer_helpers.py:81-87 + PE) -> n_layers post-LN FAVOR+ encoder layers (fast_transformer_decoder.py:54-74: fused q/k/v projection,
 *     FAVOR+ recurrent step on the fp32 state, out-projection + residual + LayerNorm, ReLU FFN + residual + LayerNorm) -> dec_out_proj logits; 128 features.
 *   form 1, GPT-2 (r06): the same loop on the GPT-2 backbone (stage2_accompaniment/model/music_gpt2.py -> HF GPT2Block: pre-LN, gelu_new, no ln_f) with
 *     the KV cache BASELINE configs[3] names.
 *   form 2, Transformer-XL (stage 1): the lead-sheet model — one token of every stream through stage1_compose/model/plain_transformer.py:52-59
 *     (PlainTransformer.generate, one-token call) -> optimus_txl_decoder.py:750-925 with attn_type 0: word embedding x emb_scale (:788), n_layers
 *     RelPartialLearnableDecoderLayer (:526-557: relative-position attention :301-391 with pre_lnorm over the last mem_len cached positions,
 *     PositionwiseFF :28-66, evaluation mode) -> dec_out_proj; the token step of the sampling loop of stage1_compose/inference_utils.py:51-134.
 *   sampled = 1 (forms 0 and 1): the NEXT token is drawn inside the launch (the sampling half of the loop of inference.py:252-277, arithmetic of
 *     emo_sample_nucleus_step: same device code): member s < 4 of a group draws stream 4 g + s from `logits` AS THE PREVIOUS STEP LEFT IT (temperature,
 *     nucleus top_p, uniform u_steps[step[r] * n_real + r]), writes the token to tok_out[r] and seq[r * ld_seq + col0 + step[r]], and the step then
 *     embeds it at position pos0 + step[r] + 1 (form 1: = the row index of the appended key); step[r] is incremented when the launch is done.
 *     Streams r >= n_real are idle padding (n_streams = n_real rounded up to 4).
 * A field that a form does not read is ignored, whatever it holds.  The struct holds raw device addresses: its owner keeps the memory alive. */
typedef struct {
    int32_t form;              /* 0 Performer, 1 GPT-2, 2 Transformer-XL */
    int32_t sampled;           /* 1: draw the token inside the launch (forms 0, 1) */
    /* --- table and shape (all forms) */
    const void* layer_table;   /* device array [n_layers][16] of pointers.
                                *   form 0: wqkv_packed, bqkv (f32 [3 d], q|k|v), wo_packed, bo, norm1 gamma, beta, w1_packed, b1, w2_packed, b2, norm2 gamma,
                                *           beta, omega (f32 [64][64]), state_S (f32 [n][8][128][64]), state_z (f32 [n][8][128]), unused.
                                *           *_packed = the bf16 nn.Linear weight [N][K] re-ordered per (member, wave 0..3 of the compute half, column tile,
                                *           k step) into 1-KB MFMA B fragments (element (lane, j) = W[16 tile + lane % 16][32 kstep + 8 (lane / 16) + j]);
                                *           the host mirror builds them (inference.py).
                                *   form 1: c_attn packed, bias (f32 [3 d]), attn.c_proj packed, bias, ln_2 gamma, beta, c_fc packed, bias, mlp.c_proj
                                *           packed, bias, ln_1 gamma, beta OF THE NEXT BLOCK (any valid pointer for the last block), unused, K cache, V cache,
                                *           unused.  Packed = the TRANSPOSED Conv1D weight ([out][in]) in the fragment order of form 0.
                                *           K / V cache: bf16 [n_streams][8][kv_tmax][64] (head-major, kv_tmax <= 2048); the step appends the token's key /
                                *           value row at index pos = pos0 + pos_ids[s] (= the number of rows already cached) and attends over rows 0 .. pos.
                                *   form 2: qkv_net packed, ZEROS (f32 [3 d]: qkv_net has no bias), o_net packed, ZEROS (f32 [d]), pos_ff.layer_norm gamma,
                                *           beta, CoreNet.0 packed, bias, CoreNet.3 packed, bias, dec_attn.layer_norm gamma, beta OF THE NEXT LAYER (any valid
                                *           pointer for the last one), R_l = r_net_l(pos_emb) (bf16 [n_dist][512], row = distance), K cache, V cache, unused.
                                *           K / V cache: bf16 [n_streams][8][kv_tmax][64], row = position; kv_tmax is NOT bounded by the 2048-entry score buffer. */
    int64_t n_layers;          /* 1 .. 15 */
    /* --- input */
    const int64_t* tok;        /* int64 [n_streams]; ignored when sampled */
    const int64_t* seg;        /* forms 0, 1: int64 [n_streams] or NULL (then Sg is not read) */
    const float* E;            /* token embedding table, f32 [n_token][512] */
    const float* Sg;           /* forms 0, 1: segment embedding table (needed when seg is given) */
    const float* pe;           /* forms 0, 1: positional table, f32 [rows][512]; form 2 has no positional and no segment table */
    float emb_scale;
    int64_t pos0;              /* forms 0, 1: position of stream s = pos0 + (pos_ids ? pos_ids[s] : 0) */
    const int64_t* pos_ids;    /* forms 0, 1: int64 [n_streams] or NULL; ignored when sampled */
    /* --- output layer (all forms) */
    const void* wout_packed;   /* dec_out_proj weight, packed as above */
    const float* bout;
    int64_t n_token;           /* <= 512 */
    float* logits;             /* f32 [n_streams][n_token]; sampled: also the logits the token is drawn from */
    /* --- sizes (all forms) */
    int64_t n_streams;         /* a multiple of 4, <= 32 */
    int64_t n_real;            /* sampled: 1 .. n_streams, the streams that draw */
    int64_t d_model, n_head;   /* 512, 8 */
    int64_t n_feat;            /* form 0: 128 */
    int64_t d_ff;              /* 2048 */
    /* --- workspace and numerics */
    void* sync_ws;             /* emo_decode_step_workspace_bytes() bytes, 16-byte aligned, ZEROED ONCE by the caller before the first step and then left
                                * alone (it carries the launch counter the granule tags are derived from); its last 8 words: [0] != 0 after a step that gave
                                * up (a workgroup could not be scheduled next to the others within 50 ms) - the caller must check it before trusting the logits. */
    int64_t sync_ws_bytes;
    float eps;                 /* form 0: the FAVOR+ normaliser's epsilon */
    float ln_eps;
    int64_t* diag;             /* NULL, or int64 [32][16][8][4] device words that receive group 0's per-phase time stamps (tools/pd_diag.py) */
    /* --- sampling (read when sampled) */
    float temperature, top_p;  /* temperature > 0 */
    const float* u_steps;      /* f32 [draws][n_real] uniforms */
    int64_t* step;             /* int64 [n_real] draw counters, advanced by the launch */
    int64_t* seq;              /* NULL, or int64 rows of ld_seq words that receive the drawn tokens at column col0 + step[r] */
    int64_t ld_seq, col0;
    int64_t* tok_out;          /* int64 [n_real] */
    /* --- form-specific */
    const float* ln0;          /* forms 1, 2: f32 [2][512]: gamma | beta of block 0's ln_1 / layer 0's dec_attn.layer_norm */
    int64_t kv_tmax;           /* forms 1, 2: rows per (stream, head) of the K / V caches; form 1: <= 2048 */
    const int64_t* lens;       /* form 2: int64 [n_streams] ON THE DEVICE: the length of each stream INCLUDING this token (the caller advances it in front
                                * of the launch); the step appends the token's key / value row at index min(lens[s] - 1, kv_tmax - 1) and attends over rows
                                * max(0, lens[s] - 1 - mem_len) .. lens[s] - 1 with the score
                                * ((q + r_w_bias[h]) . k_j + (q + r_r_bias[h]) . R_l[lens[s] - 1 - j, h]) / 8 */
    int64_t mem_len;           /* form 2: 1 <= mem_len, mem_len + 1 <= 2048 */
    int64_t n_dist;            /* form 2: rows of the R tables, >= min(mem_len, kv_tmax - 1) + 1 */
    const float* r_w_bias;     /* form 2: f32 [8][64] */
    const float* r_r_bias;     /* form 2: f32 [8][64] */
} emo_decode_step_t;
/* sizeof(emo_decode_step_t) as the library was built (a binding checks its mirror against it, as with emo_epilogue_size) */
int emo_decode_step_size(void);
int64_t emo_decode_step_workspace_bytes(void);
/* 1 when this device can hold the launch (>= 256 CUs, 96 KB of LDS per workgroup granted, one workgroup per CU by the occupancy query), else 0:
 * callers keep the chain of launches (emo_gemm + the DECODE pass of emo_attn ...) of stage2_accompaniment/inference.py:250-277 then */
int emo_decode_step_supported(void);
int emo_decode_step(const emo_decode_step_t* args, emo_stream_t stream);

/* FAVOR+ omega draw (fast-transformers orthogonal_random_matrix_, called from new_feature_map() on every
 * forward — SURVEY F8): gauss [n_layers, ceil((n_feat/2)/dh), dh, dh] ~ N(0,1) from the caller's RNG ->
 * omega [n_layers, dh, n_feat/2] with orthogonal columns per block scaled by the row norms of the block. */
int emo_favor_draw_omega(const float* gauss, float* omega, int64_t n_layers, int64_t dh, int64_t n_feat,
                         emo_stream_t stream);
/* Restart rows of the FAVOR+ recurrent state (no reference counterpart: the reference recomputes the whole prefix per token and has no state).  A
 * decode row that takes a new piece (EMO_GRAMMAR_ACC_QUEUE: row_reset, written by the grammar launch in front of this one) must start from S = 0, z = 0.
 * state_table: DEVICE array [n_layers][2] of pointers, the layer's state_S (f32 [n_rows][s_row_floats]) and state_z (f32 [n_rows][z_row_floats]), each
 * 16-byte aligned; s_row_floats = H * n_feat * dh and z_row_floats = H * n_feat, both multiples of 4.  Grid (row, layer, chunk of 4096 floats): a
 * workgroup reads row_reset[row] (int32 [n_rows]) and leaves at once when it is 0, otherwise zeroes its chunk of the row with 16-byte stores.  Rows
 * that are not flagged are not touched.  Graph-capturable; nothing is allocated. */
int emo_favor_state_reset(const void* state_table, int64_t n_layers, int64_t n_rows, int64_t s_row_floats, int64_t z_row_floats,
                          const int32_t* row_reset, emo_stream_t stream);
/* The FAVOR+ recurrent state of every row AT ITS OWN LENGTH (no reference counterpart: the state a decode row continues from after a prefill of rows
 * of different lengths, inference prefill(lens=)).  k, v: [B*T, H*dh] views with the row stride ld (elements; rows 16-byte aligned), dtype EMO_F32 or
 * EMO_BF16; omega f32 [dh, n_feat/2]; lens int32 [B] on the device, 1 <= lens[b] <= T (a value outside [0, T] is clamped: nothing outside the row is
 * read).  Per (b, h):  state_S[b,h] = sum_{t < lens[b]} phi(k_t) (x) v_t  (f32 [B,H,n_feat,dh]),  state_z[b,h] = sum_{t < lens[b]} phi(k_t)  (f32
 * [B,H,n_feat]), phi the forward's feature map (the same device function, scaling, offset and omega image) and the products on the forward's route for
 * the dtype (bf16 operands into v_mfma_f32_16x16x32_bf16 with f32 accumulation; exact f32 on v_mfma_f32_16x16x4_f32), so the state has the error class
 * of the FWD pass's state_S / state_z.  A masked reduction over tiles of 32 tokens, one workgroup per (b, h): tokens at t >= lens[b] are never loaded
 * and contribute exact zeros, whatever they hold (a tile that straddles lens[b] is masked by element, not skipped).  Built for the (d_head, n_feat)
 * rows of the FAVOR kind of emo_attn.  Graph-capturable; nothing is allocated. */
int emo_favor_state_at(const void* k, const void* v, int64_t ld, int dtype, const float* omega, const int32_t* lens, float* state_S, float* state_z,
                       int64_t B, int64_t T, int64_t H, int64_t dh, int64_t n_feat, emo_stream_t stream);

/* ------------------------------------------------------------------ K9: cross-entropy with ignore_index
 * Replaces F.cross_entropy in compute_loss (model/music_performer.py:72-81).
 * fwd: row_lse[m]; acc[0] += sum of -logp over kept rows, acc[1] += #kept rows (caller zeroes acc).
 * bwd: dlogits[m,v] = (exp(l - lse) - [v==tgt]) * (tgt!=ignore) * gscale[0]   (gscale: device scalar) */
int emo_xent_fwd(const float* logits, const int64_t* tgt, int64_t M, int64_t V, int64_t ignore_index,
                 float* row_lse, float* acc, emo_stream_t stream);
int emo_xent_bwd(const float* logits, const int64_t* tgt, const float* row_lse, const float* gscale,
                 void* dlogits, int64_t ld_out /* >= V; columns V..ld_out-1 are zero-filled */,
                 int dtype_out, int64_t M, int64_t V, int64_t ignore_index, emo_stream_t stream);

/* ------------------------------------------------------------------ K9b: per-row cross-entropy terms (sequence scoring)
 * What F.cross_entropy(..., reduction='none' / 'sum') computes — compute_loss hands `reduction` straight to it
 * (model/music_performer.py:72-81, model/music_gpt2.py:94-103) — plus the per-token figures a scoring pass reports.
 * logits: fp32 [M, ld], ld >= V; only columns < V are read (ld > V: LogitsFn's padded projection, no copy).
 * Every output is [M]; all but nll may be NULL:
 *   nll[m]     = lse[m] - logits[m, tgt[m]];  0 where tgt[m] == ignore_index (F.cross_entropy's value there)
 *   lse[m]     = log sum_v exp(logits[m, v])  (bit-identical to the row_lse of the forward above on the same values)
 *   rank[m]    = #{v : l[v] > l[tgt]} + #{v < tgt : l[v] == l[tgt]}: 0 exactly where the argmax below returns tgt[m]
 *                ("first max wins");  -1 on ignored rows
 *   entropy[m] = lse - sum_v softmax(l)_v l_v  in nats, ignored rows included
 * bwd_rows: dlogits[m,v] = (exp(l - lse) - [v==tgt]) * (tgt!=ignore) * grow[m]   (grow: fp32 [M], the upstream gradient of nll) */
int emo_token_scores(const float* logits, int64_t ld, const int64_t* tgt, int64_t M, int64_t V, int64_t ignore_index,
                     float* nll, float* lse, int32_t* rank, float* entropy, emo_stream_t stream);
int emo_xent_bwd_rows(const float* logits, int64_t ld, const int64_t* tgt, const float* row_lse, const float* grow,
                      void* dlogits, int64_t ld_out /* >= V; columns V..ld_out-1 are zero-filled */,
                      int dtype_out, int64_t M, int64_t V, int64_t ignore_index, emo_stream_t stream);

/* ------------------------------------------------------------------ K10/K12: sampling + accuracy
 * argmax over V per row (greedy / parity mode; first max wins like np.argmax / torch.argmax).
 * nucleus: softmax(l/temp) -> sort desc -> keep through the token that crosses top_p
 * (inference.py:71-100 semantics incl. F12) -> renormalise -> draw from u[row] in [0,1). */
int emo_argmax(const float* logits, int64_t rows, int64_t V, int64_t* out, emo_stream_t stream);
int emo_sample_nucleus(const float* logits, int64_t rows, int64_t V, float temperature, float top_p,
                       const float* u, int64_t* out, emo_stream_t stream);
/* One step of the lock-step generation loop (inference.py:252-327 with grammar checks off) with all loop state on the device, so
 * the step can be captured once in a hipGraph and replayed: stream r draws with u_steps[step[r], r] (u_steps: [n_steps, rows]),
 * the sampled id goes to out[r] and to seq[r, col0 + step[r]] (seq may be NULL), then step[r] += 1. */
int emo_sample_nucleus_step(const float* logits, int64_t rows, int64_t V, float temperature,
                            float top_p, const float* u_steps, int64_t* step, int64_t* seq,
                            int64_t ld_seq, int64_t col0, int64_t* out, emo_stream_t stream);
/* EMO_GRAMMAR_TXL.  Stage-1 lead-sheet generation (stage1_compose/inference_utils.py generate_plain_xl :51-134, match_emotion_key :137-142): the draw and the
 * grammar of one lock-step token step for n streams, one 512-thread workgroup per stream, all loop state in device memory (graph-capturable).
 * A stream that is RUNNING and has fed its whole primer (state[FEED] >= params[PRIMER_LEN]) draws from logits[r] (fp32 [n, V], V <= 1024) with
 * uniform u_steps[state[DRAWS] * n + r] (u_steps [n_u, n]) — the device code of emo_sample_nucleus, so the same id —, at key_temperature /
 * key_top_p when params[KEYED] and the stream holds exactly one token (reference: 1.1 / 0.97), else at temperature / top_p.  Then, in the
 * reference's order: the key rule (params[KEY_RULE], key draw only: a non-Key event -> KEY_ERROR; a key whose mode contradicts params[EMO_MODE]
 * is rejected), Beat (a position below state[BEAT] is rejected and counted, 256 in a row -> STUCK; accepted: count reset), Bar (bars += 1,
 * position 0), PAD (rejected, not counted), append to seq[r] (int64, pitch ld_seq; DONE when the length exceeds params[MAX_EVENTS] or the
 * event is EOS), DONE when bars >= params[MAX_BARS].  tok_out[r] = the next input: the accepted word; after a rejection the previous input
 * again; after a rejection with nothing accepted the primer (seq[r, 0 .. PRIMER_LEN)) again, one token per step with no draws.  A stream still
 * feeding its primer writes tok_out[r] = seq[r, FEED] and advances FEED; a stream that finishes leaves its last token in tok_out[r] (its row
 * idles).  *running is decremented once per stream that leaves RUNNING.
 * ev_flags [V] (EMO_TXL_EV_* bits: 'Beat' in e, 'Bar' in e, e == 'PAD_None', e == 'EOS_None', e.split('_')[0] == 'Key', the key's tonic in
 * MAJOR_KEY / MINOR_KEY) and ev_beat [V] (int(e.split('_')[-1]) of Beat events) are built on the host from idx2event.
 * Optional kept bars (keep_tok / keep_beg / keep_end / keep_left, the comment of the fields below): a bar the caller already has is written out,
 * not drawn, in the launch that accepts the Bar in front of it, and fed one token per launch; rows then need the longest kept run on top.
 * params int32 [n, EMO_TXL_PARAM_WORDS], state int32 [n, EMO_TXL_STATE_WORDS], laid out as the enums below. */
enum { EMO_TXL_P_MAX_BARS = 0, EMO_TXL_P_MAX_EVENTS = 1, EMO_TXL_P_PRIMER_LEN = 2, EMO_TXL_P_KEYED = 3, EMO_TXL_P_KEY_RULE = 4,
       EMO_TXL_P_EMO_MODE = 5 /* 0 none, 1 major (Q1 / Q4 / Positive), 2 minor (Q2 / Q3 / Negative) */,
       EMO_TXL_P_KEEP0 = 6 /* kept bars: the stream's first entry of keep_beg / keep_end */, EMO_TXL_P_KEEP_BARS = 7 /* and how many it has (0: none) */,
       EMO_TXL_PARAM_WORDS = 8 };
enum { EMO_TXL_S_STATUS = 0, EMO_TXL_S_LEN = 1 /* tokens in seq[r] */, EMO_TXL_S_ACCEPTED = 2, EMO_TXL_S_BEAT = 3, EMO_TXL_S_BARS = 4,
       EMO_TXL_S_FAILED = 5 /* rejected Beats in a row */, EMO_TXL_S_FEED = 6 /* next primer token to feed */, EMO_TXL_S_DRAWS = 7, EMO_TXL_STATE_WORDS = 8 };
enum { EMO_TXL_RUNNING = 0, EMO_TXL_DONE = 1, EMO_TXL_STUCK = 2, EMO_TXL_KEY_ERROR = 3, EMO_TXL_OVERFLOW = 4 /* seq or u_steps exhausted */,
       EMO_TXL_MEM_FULL = 5 /* TXL_QUEUE: the slot's row of the model's memory has no place for another token */ };
enum { EMO_TXL_EV_BEAT = 1, EMO_TXL_EV_BAR = 2, EMO_TXL_EV_PAD = 4, EMO_TXL_EV_EOS = 8, EMO_TXL_EV_KEY = 16, EMO_TXL_EV_MAJOR = 32, EMO_TXL_EV_MINOR = 64 };
/* EMO_GRAMMAR_ACC.  Stage-2 accompaniment generation (stage2_accompaniment/inference.py generate_conditional :231-327): the draw and the grammar of one lock-step
 * token step for n streams, one 512-thread workgroup per stream, all loop state in device memory (graph-capturable).  seq / segs (int64, pitch
 * ld_seq) hold each stream's `generated` / segment ids; state[LEN] of them are valid, state[CONSUMED] have been fed to the model.  Per stream r:
 *   not RUNNING                 -> tok_out[r] = pad, seg_out[r] = 1;
 *   state[LEN] >= max_len       -> WINDOW (the reference's window slides at max_dec_inp_len), then as above;
 *   state[CONSUMED] < state[LEN] -> tok_out[r] / seg_out[r] = seq / segs[r, CONSUMED], CONSUMED += 1 (no draw);
 *   otherwise draw from logits[r] (fp32 [n, V], V <= 1024) with u_steps[state[DRAWS] * n + r] (u_steps [n_u, n]; the device code of
 *   emo_sample_nucleus, so the same id), DRAWS += 1, and run the grammar of the reference: with params[SKIP_CHECK] == 0 a Beat below
 *   state[CUR_POS] is rejected and counted (256 in a row -> STUCK; accepted: CUR_POS = its position, count reset); Track_LeadSheet is appended
 *   with segment 0 and BARS += 1, then below params[TARGET_BARS] the next lead-sheet bar (segment 0) and track_full (segment 1) are appended
 *   and CUR_POS = 0, else DONE; PAD, and EOS before the last bar, are rejected (not counted); EOS at the last bar is appended and DONE; any
 *   other event is appended with segment 1 (DONE when the length exceeds params[MAX_EVENTS]).  A rejected sample is drawn again from the same
 *   logits with the next uniform INSIDE the launch (the reference's `continue`), until an acceptance, STUCK or the end of the table
 *   (OUT_OF_DRAWS).  A stream still RUNNING then feeds seq[r, CONSUMED] as above; one that finished feeds pad.  *running is decremented once
 *   per stream that leaves RUNNING.
 * ev_flags [V] (EMO_ACC_EV_* bits: 'Beat' in e, e == 'Track_LeadSheet', e == 'PAD_None', e == 'EOS_None') and ev_beat [V] (beat_position of
 * Beat events) are built on the host from idx2event.  Lead sheets: lead_tok int64 (all bars of all streams, flat) and lead_off int32: bar j of
 * stream r is lead_tok[lead_off[params[BAR0] + j] .. lead_off[params[BAR0] + j + 1]), j < params[N_BARS].  Rows of width >= max_len + the
 * longest bar + 2 always hold an injected bar; a row or a bar table too short for a step is a caller error (OVERFLOW).
 * Optional kept bars (keep_tok / keep_beg / keep_end, the comment of the fields below): a bar the caller already has is written out, not drawn, in
 * the launch that accepts the Track_LeadSheet in front of it, and fed like an injected lead-sheet bar; rows then need the longest kept run on top.
 * params int32 [n, EMO_ACC_PARAM_WORDS], state int32 [n, EMO_ACC_STATE_WORDS], laid out as the enums below. */
enum { EMO_ACC_P_TARGET_BARS = 0, EMO_ACC_P_MAX_EVENTS = 1, EMO_ACC_P_SKIP_CHECK = 2, EMO_ACC_P_BAR0 = 3, EMO_ACC_P_N_BARS = 4, EMO_ACC_PARAM_WORDS = 8 };
enum { EMO_ACC_S_STATUS = 0, EMO_ACC_S_LEN = 1 /* tokens in seq[r] */, EMO_ACC_S_CONSUMED = 2 /* tokens fed to the model */,
       EMO_ACC_S_BARS = 3 /* generated_bars */, EMO_ACC_S_CUR_POS = 4, EMO_ACC_S_FAILED = 5 /* rejected Beats in a row */, EMO_ACC_S_DRAWS = 6,
       EMO_ACC_S_ACCEPTED = 7 /* accepted draws */, EMO_ACC_STATE_WORDS = 8 };
enum { EMO_ACC_RUNNING = 0, EMO_ACC_DONE = 1, EMO_ACC_STUCK = 2, EMO_ACC_WINDOW = 3, EMO_ACC_OUT_OF_DRAWS = 4, EMO_ACC_OVERFLOW = 5 };
enum { EMO_REBASE_BAR_TOO_LONG = 6 };   /* a further value of state[STATUS], written by emo_acc_rebase alone: no grammar step ever writes it, all read it as finished */
enum { EMO_ACC_EV_BEAT = 1, EMO_ACC_EV_TRACK_LS = 2, EMO_ACC_EV_PAD = 4, EMO_ACC_EV_EOS = 8 };
/* EMO_GRAMMAR_ACC_WINDOW.  The same draw and grammar for streams PAST the window (stage2_accompaniment/inference.py:252-277: the model input is the last max_dec_inp_len
 * tokens of `generated`, positions restarting at 0 on every step, so nothing is fed token by token and an injected bar is simply part of the next
 * input): one forward over [m, window] per draw, then this launch.  Row b of the batch (logits fp32 [m, V], win_tok / win_seg int64 [m, window])
 * belongs to stream r = rows[b] (int32 [m]; NULL: r = b), which indexes params, state, seq, segs and the column of u_steps (fp32 [n_u, ld_u],
 * ld_u = the number of streams; the uniform of draw d of stream r is u_steps[d * ld_u + r]), so a caller may drop finished rows from the batch
 * without moving any state.  A row whose r is outside [0, ld_u) is skipped.
 *   not RUNNING                 -> nothing is drawn, win_tok / win_seg[b] stay as they are;
 *   state[LEN] < window         -> OVERFLOW (a caller error: there is no full window to read);
 *   otherwise the draw, the in-launch redraws and the grammar of the ACC kind (the same device code), state[CONSUMED] untouched; a
 *   stream still RUNNING then gets its next model input, win_tok / win_seg[b, 0 .. window) = seq / segs[r, LEN - window .. LEN).
 * OUT_OF_DRAWS, OVERFLOW (ld_seq too short for the accepted tokens) and *running behave as in the ACC kind. */
/* EMO_GRAMMAR_TXL_QUEUE.  The TXL kind for MORE JOBS THAN ROWS: the n_rows rows of the model batch are SLOTS, the streams are n_jobs JOBS waiting in a queue, and
 * a slot whose job ends takes the next one inside the launch, so that no host round trip (and no break in a hipGraph replay) lies between two
 * jobs of a row.  One 512-thread workgroup per slot b, which owns logits[b], tok_out[b] and mem_lens[b] (the per-row length of the model's
 * memory: a Transformer-XL row restarts when its length is 0) and works on job j = slot_job[b] (int32 [n_rows]; -1: free).  Everything the TXL
 * kind indexes by stream is indexed by job: params, state, seq, the score tables (n_jobs rows each) and the column of u_steps (ld_u = n_jobs;
 * draw d of job j takes u_steps[d * ld_u + j]).  Per launch and slot:
 *   slot_job[b] = a RUNNING job -> if mem_lens[b] >= mem_rows the job ends with MEM_FULL (the per-row form of the lock-step loop's bound:
 *                                  the row cannot take the token of another step); otherwise exactly the TXL kind's step for stream j (the same
 *                                  device code): primer feed, draw, key rule, Beat / Bar / PAD / EOS, the limits, the re-feeds, the scores;
 *   slot_job[b] free, or the job left RUNNING in this launch -> thread 0 takes jobs from the queue (h = atomicAdd(queue_head, 1), h < n_jobs)
 *                                  until one is RUNNING (a job the host closed before the run is passed over).  With a job j': slot_job[b] = j',
 *                                  mem_lens[b] = 0, tok_out[b] = seq[j', 0], state[j', FEED] = 1: the model step behind this very launch is
 *                                  the job's first token, no step idles in between.  With the queue empty: slot_job[b] = -1 and mem_lens[b] = 0,
 *                                  in this and in every later launch (queue_head is not added to again), so the model step, which still runs
 *                                  on the row, stays at the first row of its cache.
 * The first launch starts from slot_job = -1 everywhere, queue_head = 0, mem_lens = 0 and tok_out = any valid id, and admits the first jobs
 * itself: every primer token goes through the one-token model step (state[j, FEED] as the host leaves it is ignored).  *running starts at the
 * number of RUNNING jobs and is decremented once per job.  Which of several slots that free up in one launch gets which job is not specified; a
 * job's ids depend on the job (its rows, its uniform column, its counters) and the logits it is shown, nothing else.  job_steps (int32 [n_jobs]
 * or NULL): when a job ends, job_steps[j] = mem_lens[b] = the tokens the model was fed for it = the launches it held its slot. */
/* EMO_GRAMMAR_ACC_QUEUE.  The ACC kind for MORE JOBS THAN ROWS, as TXL_QUEUE is for TXL: the n_rows rows of the model batch are SLOTS, the streams are n_jobs JOBS
 * waiting in a queue, and a slot whose job ends takes the next one inside the launch.  One 512-thread workgroup per slot b, which owns logits[b],
 * tok_out[b], seg_out[b], mem_lens[b] and row_reset[b] and works on job j = slot_job[b] (int32 [n_rows]; -1: free).  Everything the ACC kind indexes by
 * stream is indexed by job: params, state, seq, segs, the score tables (n_jobs rows each) and the column of u_steps (ld_u >= n_jobs; draw d of job j takes
 * u_steps[d * ld_u + j]).  The queue fields are TXL_QUEUE's with the ACC meaning: mem_lens (int64 [n_rows]) is the POSITION of the token each row is fed in
 * the model step behind the launch (the decode engine's device position array: the positional-table row and, for a KV cache, the row the token's key is
 * appended at, so a row restarts by being fed position 0), mem_rows the position bound (min(max_len, rows of the positional table)).  Per launch and slot:
 *   slot_job[b] = a RUNNING job -> state[LEN] >= max_len: WINDOW, as in the ACC kind; otherwise state[CONSUMED] >= mem_rows: OVERFLOW (the token of this
 *                                  step has no position; a caller whose table has max_len rows never sees it); otherwise exactly the ACC kind's step for
 *                                  stream j (the same device code): the feed of a pending token, the draw, the in-launch redraws, the grammar, the bar
 *                                  injection, the scores.  The token fed is seq[j, CONSUMED - 1] after the step: mem_lens[b] = CONSUMED - 1, row_reset[b] = 0;
 *   slot_job[b] free, or the job left RUNNING in this launch (DONE, STUCK, WINDOW, OUT_OF_DRAWS, OVERFLOW) -> job_steps[j] = state[j, CONSUMED] = the tokens
 *                                  the model was fed for it = the launches it held its slot; then thread 0 takes jobs from the queue (h =
 *                                  atomicAdd(queue_head, 1), h < n_jobs) until one is RUNNING (a job the host closed before the run is passed over).  With
 *                                  a job j': slot_job[b] = j', row_reset[b] = 1, state[j', CONSUMED] = 1, tok_out[b] / seg_out[b] = seq / segs[j', 0],
 *                                  mem_lens[b] = 0: the model step behind this very launch is the job's first token.  With the queue empty: slot_job[b] =
 *                                  -1, row_reset[b] = 0, tok_out[b] = pad, seg_out[b] = 1, mem_lens[b] = 0, in this and in every later launch (queue_head
 *                                  is not added to again).
 * row_reset (int32 [n_rows]) is written in EVERY launch: 1 for a slot that admitted a job in it, else 0.  A model whose rows carry state besides the
 * cache that position 0 overwrites (the Performer's S / z) clears the flagged rows between this launch and its step: emo_favor_state_reset.  The first
 * launch starts from slot_job = -1 everywhere and queue_head = 0 and admits the first jobs itself: there is no prefill, every primer token goes through the
 * one-token step (state[j, CONSUMED] as the host leaves it is ignored).  *running starts at the number of RUNNING jobs and is decremented once per job. */
/* The five grammar steps above are the kinds of ONE entry with ONE argument block, as emo_decode_step_t is for the model step beside them in
 * every generation loop.  `kind` selects the kernel; a field that a kind does not read is ignored by it, whatever it holds (the comment of each
 * field names its readers; none = all five, as are the optional sampling controls and score outputs at the end of the block; a field of TXL is a field of TXL_QUEUE too, a field of ACC a field of ACC_QUEUE, where the field's comment does not say otherwise).  The block is read AT CALL TIME: its values travel as the launch's arguments, so under hipGraph
 * capture they are baked into the captured launch, exactly as positional arguments would be, and a later change of the block reaches only later
 * calls (and later captures).  The struct holds raw device addresses: its owner keeps the memory alive. */
enum { EMO_GRAMMAR_TXL = 0, EMO_GRAMMAR_ACC = 1, EMO_GRAMMAR_ACC_WINDOW = 2, EMO_GRAMMAR_TXL_QUEUE = 3, EMO_GRAMMAR_ACC_QUEUE = 4 };   /* what each does: the five comments above (n = n_rows, V = n_token) */
typedef struct {
    int32_t kind;              /* EMO_GRAMMAR_* */
    /* --- all kinds */
    int64_t n_rows;            /* workgroups launched: TXL, ACC the n streams; ACC_WINDOW the m rows of the batch; TXL_QUEUE, ACC_QUEUE the slots */
    const float* logits;       /* f32 [n_rows, n_token] */
    int64_t n_token;           /* V <= 1024 */
    float temperature, top_p;  /* temperature > 0 */
    const float* u_steps;      /* f32 [n_u, ld_u] uniforms: draw d of stream r takes u_steps[d * ld_u + r] */
    int64_t n_u, ld_u;         /* ld_u = the number of streams (TXL, ACC: >= n_rows; TXL_QUEUE, ACC_QUEUE: >= n_jobs) */
    const int32_t* ev_flags;   /* int32 [n_token]: EMO_TXL_EV_* / EMO_ACC_EV_* bits */
    const int32_t* ev_beat;    /* int32 [n_token] */
    const int32_t* params;     /* int32 [streams, 8] */
    int32_t* state;            /* int32 [streams, 8] */
    int64_t* seq;              /* int64 [streams, ld_seq] */
    int64_t ld_seq;
    int32_t* running;          /* int32 [1] */
    /* --- kind-specific (ordered so that the fields one kind reads lie together: a kernel fetches its arguments in runs) */
    float key_temperature, key_top_p;   /* TXL: the key draw; key_temperature > 0 */
    int64_t* tok_out;          /* TXL, ACC: int64 [n_rows] */
    int64_t* seg_out;          /* ACC: int64 [n_rows] */
    int64_t max_len;           /* ACC: > 0 */
    int64_t pad;               /* ACC */
    /* (kinds ACC and TXL, the two lock-step kinds - ACC_QUEUE, TXL_QUEUE and ACC_WINDOW ignore the three, whatever they hold; all three or none;
     * all NULL: the launch is exactly the one without them.)  Classifier-free guidance over a MIRRORED PAIR of streams of the batch.  Stream r is guided when guide_cond[r] = c
     * and guide_uncond[r] = g are two distinct values in [0, n_rows); any other pair of values is "unguided" to the kernel, which never reads
     * outside the tables.  A guided stream draws from l[v] = lc + s * (lc - lu), lc = logits[c, v], lu = logits[g, v], s = guide_scale[r]: three
     * separately rounded fp32 operations, never contracted, so NumPy's float32 `lc + s * (lc - lu)` is the same row bit for bit; the stream's ban
     * is applied AFTER the combination (a banned token is -INFINITY, no inf - inf arises from it; the logits themselves are finite); s = 0 is
     * row c itself.  Its uniforms come from column c of u_steps.  The leader of a pair is c (the conditioned primer), its follower g (the same
     * primer with the unconditioned token in the condition's place); both carry the same (c, g, s), equal temp / top_p / ban, and run the same
     * grammar on the same draw in their own workgroups: the follower stays token for token with its leader without any traffic between the two,
     * and every row writes only its own tok_out / seg_out / state / seq / segs.  tok_logp / tok_rank / tok_entropy stay the model's figures from
     * the row's OWN logits at temperature 1: the leader's are the conditioned model's, the follower's the unconditioned model's for the same
     * tokens.  The host owns the checks that need the values (ops.block_set: indices in range, pairs consistent, 0 <= s < inf).
     * Kind TXL (stage 1: the condition is the valence tag, the follower's primer holds Emotion_None in its place): the same, the key draw
     * included (the combination at key_temperature / key_top_p).  A TXL stream has one draw per launch and a rejection re-feeds an input, so the
     * pair also shares every rejection: the follower's params[EMO_MODE] is its LEADER's (the key rule then rejects for both or for neither), and
     * the draw runs under the controls of row c.  There is no seg_out / segs to speak of. */
    const int32_t* guide_cond;    /* ACC, TXL (not TXL_QUEUE): int32 [n_rows] or NULL: the row whose logits are the conditioned ones for stream r, or -1 */
    const int32_t* guide_uncond;  /* ACC, TXL (not TXL_QUEUE): int32 [n_rows] or NULL: the row whose logits are the unconditioned ones, or -1 */
    const float* guide_scale;     /* ACC, TXL (not TXL_QUEUE): f32 [n_rows] or NULL: s >= 0 */
    int64_t* segs;             /* ACC, ACC_WINDOW: int64 [streams, ld_seq] */
    const int64_t* lead_tok;   /* ACC, ACC_WINDOW */
    const int32_t* lead_off;   /* ACC, ACC_WINDOW */
    /* (kinds ACC and ACC_QUEUE - ACC_WINDOW ignores the five, whatever they hold, and kinds TXL / TXL_QUEUE read the first four their own way: the comment behind keep_eos; the three tables come together or not at
     * all; all NULL: the launch is exactly the one without them.)  KEPT BARS: accompaniment bars the caller already has.  keep_beg / keep_end are
     * indexed like lead_off, by params[BAR0] + j, j < params[N_BARS] (one entry per lead-sheet bar: the host checks the lengths against
     * lead_off's); keep_beg < 0: bar j is drawn, as ever; otherwise its accompaniment is keep_tok[keep_beg .. keep_end), possibly empty (a kept
     * empty bar is not a drawn bar), without the Track_Full before it and the Track_LeadSheet / EOS behind it.  A range outside [0, n_keep] or
     * running backwards ends the stream OVERFLOW: nothing outside keep_tok is read.  When an accepted Track_LeadSheet opens bar j (the next
     * lead-sheet bar and track_full appended) and bar j is kept, thread 0 goes on in the same launch: the kept tokens with segment 1 (the
     * length test against params[MAX_EVENTS] after each one, DONE inside the bar where it fires; no Beat check, no PAD / EOS rejection); then,
     * for a bar that is not the last of params[TARGET_BARS], the Track_LeadSheet id with segment 0, BARS += 1 and the opening of bar j + 1 (a
     * chain through consecutive kept bars), for the last one keep_eos with segment 1 and DONE.  The chain is walked once without writing: if it
     * does not fit ld_seq the stream ends OVERFLOW with its row, LEN, BARS, ACCEPTED and DRAWS as before the draw (without a kept bar behind
     * the Track_LeadSheet the overflowing draw stays counted, as ever).  ACCEPTED and DRAWS move for the drawn Track_LeadSheet alone, the score cell is its
     * cell; kept tokens lie in seq / segs beyond CONSUMED and are fed one per launch like an injected lead-sheet bar.  CUR_POS is 0 at the bar
     * that is next opened for drawing, and FAILED is 0 there when a kept bar lay in between (without one it is carried, as ever).  Kept bars at
     * the start of a piece are in the row when the host loads it (inference._Stream is the rule on the host). */
    const int64_t* keep_tok;   /* ACC, ACC_QUEUE, TXL, TXL_QUEUE: int64 [n_keep] or NULL: all kept bars of all streams, flat */
    const int32_t* keep_beg;   /* ACC, ACC_QUEUE: int32 [bars of lead_off] or NULL: < 0 = the bar is drawn; TXL, TXL_QUEUE: int32 [all streams' kept-bar entries] */
    const int32_t* keep_end;   /* ACC, ACC_QUEUE: int32 [bars of lead_off] or NULL; TXL, TXL_QUEUE: as keep_beg */
    int64_t n_keep;            /* ACC, ACC_QUEUE, TXL, TXL_QUEUE: entries of keep_tok */
    int64_t keep_eos;          /* ACC, ACC_QUEUE: the id that closes a kept last bar (EOS_None) */
    /* (kinds TXL and TXL_QUEUE read the four fields keep_tok / keep_beg / keep_end / n_keep above and the two below; the three tables and keep_left
     * come together or not at all; all NULL: the launch is exactly the one without them.)  KEPT BARS of a lead sheet.  Stream r (a job, for
     * TXL_QUEUE) has params[KEEP_BARS] entries of keep_beg / keep_end from params[KEEP0] on, indexed by the BAR NUMBER j: bar j is the bar opened
     * by the Bar event that is accepted while state[BARS] == j (BARS then becomes j + 1; a primer's own bars are never kept).  keep_beg < 0, or
     * j >= params[KEEP_BARS]: the bar is drawn, as ever; otherwise its content is keep_tok[keep_beg .. keep_end), possibly empty, with neither
     * Bar.  KEEP0 < 0 or KEEP_BARS <= 0 is "no kept bars" to the kernel; the host checks KEEP0 + KEEP_BARS against the tables' length
     * (ops.block_set).  When a drawn Bar has been accepted and appended, has opened bar j and left the stream RUNNING, and bar j is kept, thread
     * 0 goes on in the same launch: the kept tokens (the length test against params[MAX_EVENTS] after each one, DONE inside the bar where it
     * fires; no Beat check, no PAD / EOS rejection), then keep_bar, the Bar that closes it and opens bar j + 1: BARS += 1, the length test, DONE
     * when BARS has reached params[MAX_BARS] (the closing Bar a caller drops, as it drops a drawn one); else a chain through consecutive kept
     * bars.  The chain is walked once without writing: a range outside [0, n_keep], a range running backwards, or a chain that does not fit
     * ld_seq ends the stream OVERFLOW with its row, LEN, BARS, BEAT, FAILED, ACCEPTED and DRAWS as before the draw (the reading of kinds ACC /
     * ACC_QUEUE: the overflowing draw is not counted), and nothing outside keep_tok is read.  ACCEPTED and DRAWS move for the drawn Bar alone, the
     * score cell is its cell.  The launch feeds the drawn Bar (tok_out); keep_left[r] = the tokens the chain wrote, which lie in seq[r] below LEN
     * and are not yet fed: a RUNNING stream past its primer feed with keep_left[r] > 0 writes tok_out = seq[r, LEN - keep_left[r]], decrements
     * keep_left[r] and does not draw, so the next draw is made from the logits behind the last forced Bar, and a rejection there feeds that Bar
     * again.  BEAT and FAILED are 0 at the bar that is next opened for drawing.  A stream that ends inside the chain has keep_left[r] = 0 and
     * leaves its last token in tok_out.  TXL_QUEUE: the fed kept tokens count against mem_rows like any other (MEM_FULL), and job_steps includes
     * them.  A guided pair carries the same kept bars in both rows (the same KEEP0 / KEEP_BARS): each row writes its own chain.
     * stage1_inference._LeadSheet._open_bar is the rule on the host. */
    int64_t keep_bar;          /* TXL, TXL_QUEUE: the id that closes a kept bar (Bar_None), in [0, n_token) where the tables are present */
    int32_t* keep_left;        /* TXL, TXL_QUEUE: int32 [streams] or NULL: kept tokens written in the row and not yet fed; the caller starts it at 0 */
    int64_t track_full;        /* ACC, ACC_WINDOW */
    int64_t window;            /* ACC_WINDOW: 0 < window <= ld_seq */
    const int32_t* rows;       /* ACC_WINDOW: int32 [n_rows] or NULL */
    int64_t* win_tok;          /* ACC_WINDOW: int64 [n_rows, window] */
    int64_t* win_seg;          /* ACC_WINDOW: int64 [n_rows, window] */
    /* --- all kinds (TXL, ACC, ACC_WINDOW, TXL_QUEUE, ACC_QUEUE read all five fields), optional SOFT sampling controls, per stream and indexed
     * like tok_mask / temp_of / top_p_of below (they stand in front of the queue kinds' fields: the tail of the block stays as it is);
     * NULL: absent; with these and those four all NULL the launch is exactly the one without them.  Like the ban they
     * reach the DRAW alone: primer tokens, injected lead-sheet bars, kept bars and track_full are fed as they are, and tok_logp / tok_rank /
     * tok_entropy (and the host's logp_uncond) stay the model's own, from the unbiased row at temperature 1.
     * BIAS: the draw of stream r reads the logit of token c as l(c) + tok_bias[bias_of[r], c]: ONE rounded fp32 add, never contracted, so
     * the id, every state word, seq and segs are bit for bit those of the launch without a bias on a logits row that NumPy's float32 `l + b`
     * wrote.  Under guidance the bias is added AFTER the three-operation combination, with the LEADER's bias row for both rows of a pair;
     * the ban is applied last.  (Kind TXL takes every control of a guided draw from the leader's row; kind ACC takes the bias row from
     * the leader and the ban, temp, top_p, top_k and min_p from the row itself.  The host refuses a pair whose rows differ, so the two
     * rules give the same draw.)  Values are finite or -INFINITY (-inf behaves as a ban); +inf and NaN are refused by the host.
     * CUTS: with `last` the candidate count top-p gives (second crossing; single crossing: all; no crossing: top 3), the draw keeps
     * min(last, k, n_m) candidates of the ranking (probability descending, ties by ascending index: a tie group that straddles k keeps its
     * lowest indices): k = top_k_of[r], k <= 0 off, k = 1 greedy under that tie rule, k >= n_token no cut; n_m = max(1, #{i : sp[i] >= m *
     * sp[0]}) over the sorted fp32 probabilities, m = min_p_of[r], the product one rounded fp32 multiply, m <= 0 off, m > 1 leaves the best
     * token alone.  The f64 renormalisation and the draw run over the final count, and so do the in-launch redraws of ACC / ACC_WINDOW.
     * The TXL key draw keeps key_temperature / key_top_p and runs under the bias and both cuts, as it runs under the ban. */
    const float* tok_bias;     /* f32 [n_biases, n_token] or NULL: shared bias rows; needs bias_of and n_biases > 0 */
    int64_t n_biases;          /* rows of tok_bias */
    const int32_t* bias_of;    /* int32 [streams] or NULL: the row of tok_bias each stream draws under; a value outside [0, n_biases) = no bias: the
                                * kernel never reads outside the table (ops.block_set refuses a value outside [-1, n_biases)).  Without tok_bias it is not read */
    const int32_t* top_k_of;   /* int32 [streams] or NULL: the rank cap k per stream; <= 0 = off */
    const float* min_p_of;     /* f32 [streams] or NULL: the floor m relative to the best probability per stream; <= 0 = off */
    /* (the queue kinds alone, TXL_QUEUE and ACC_QUEUE; the last of the kind-specific fields: the optional outputs below stay the tail of the block) */
    int32_t* slot_job;         /* queue kinds: int32 [n_rows]: the job of each slot, -1 = free */
    int32_t* queue_head;       /* queue kinds: int32 [1]: the next job to hand out */
    int64_t n_jobs;            /* queue kinds: rows of params, state, seq (segs) and the score tables; 0 < n_jobs <= ld_u */
    int64_t* mem_lens;         /* TXL_QUEUE: int64 [n_rows]: the per-row lengths of the model's memory (the array the model step advances);
                                * ACC_QUEUE: int64 [n_rows]: the per-row positions the model step reads (the decode engine's pos_dev) */
    int64_t mem_rows;          /* TXL_QUEUE: cache rows per row of the memory, > 0; ACC_QUEUE: the position bound, > 0 */
    int32_t* job_steps;        /* queue kinds: int32 [n_jobs] or NULL: per finished job, the launches it held a slot */
    /* --- all kinds, optional sampling controls (in front of row_reset: row_reset and the outputs below stay the tail of the block; NULL:
     * absent; all four NULL: the launch is exactly the one without them).  Per STREAM, indexed as params is: by the stream r (TXL, ACC), by
     * the job (TXL_QUEUE, ACC_QUEUE), by r = rows[b] (ACC_WINDOW).  They reach the DRAW alone: the
     * draw reads a banned token's logit as -INFINITY and otherwise runs the arithmetic it always runs, so the id, every state word, seq and
     * segs are bit for bit those of the launch without a mask on logits whose banned entries were overwritten with -inf (the in-launch redraws
     * of ACC / ACC_WINDOW reuse the masked sort).  Primer tokens, injected lead-sheet bars and track_full are fed as they are, banned or not.
     * tok_logp / tok_rank / tok_entropy below are still taken from the model's UNMASKED logits row at temperature 1: they say what the model
     * assigned to the drawn token, not what the constraint left of the distribution.  The host owns the checks the launch cannot make (a
     * temp_of value > 0, a top_p_of value in (0, 1], a mask that leaves a token): the kernel reads nothing out of bounds whatever they hold. */
    const uint32_t* tok_mask;  /* uint32 [n_masks, ceil(n_token / 32)] or NULL: bit v & 31 of word v >> 5 of a row set = token v is banned for draws
                                * (bits at or beyond n_token in the last word are ignored) */
    int64_t n_masks;           /* rows of tok_mask */
    const int32_t* mask_of;    /* int32 [streams] or NULL: the row of tok_mask each stream draws under; -1 = none, and so is any value outside
                                * [-1, n_masks) to the kernel, which never reads outside the table (ops.block_set refuses such a value).  Without tok_mask it is not read */
    const float* temp_of;      /* f32 [streams] or NULL: replaces `temperature` per stream (the TXL key draw keeps key_temperature) */
    const float* top_p_of;     /* f32 [streams] or NULL: replaces `top_p` per stream (the TXL key draw keeps key_top_p) */
    int32_t* row_reset;        /* ACC_QUEUE: int32 [n_rows], written every launch: 1 where the slot admitted a job in this launch, else 0 */
    /* --- all kinds, optional (NULL: not wanted; all three NULL: the launch is exactly the one without them).  What the model assigned to each
     * DRAWN token, taken from the logits row the draw was made from: tables [streams, ld_seq] laid out like seq.  When a draw is accepted and
     * appended at seq[r, c], cell [r, c] gets the figures of emo_token_scores (K9b) for that token at TEMPERATURE 1, whatever temperature the
     * draw used (the TXL key draw included): logp = l[tok] - lse, rank = #{v : l[v] > l[tok]} + #{v < tok : l[v] == l[tok]}, entropy = lse -
     * sum_v softmax(l)_v l_v.  No other cell is ever written: not a primer token, not an injected lead-sheet bar or track_full, not a rejected
     * draw (ACC, ACC_WINDOW redraw inside the launch and record the accepted word only), not a step that ends in STUCK, OVERFLOW, OUT_OF_DRAWS,
     * KEY_ERROR or WINDOW.  The caller pre-fills the tables (NaN / -1, say): the cells still holding its value are the tokens that were given. */
    float* tok_logp;           /* f32 [streams, ld_seq] or NULL */
    int32_t* tok_rank;         /* int32 [streams, ld_seq] or NULL */
    float* tok_entropy;        /* f32 [streams, ld_seq] or NULL */
} emo_grammar_step_t;
/* sizeof(emo_grammar_step_t) as the library was built (a binding checks its mirror against it, as with emo_epilogue_size) */
int emo_grammar_step_size(void);
/* Messages name the kind: "emo_grammar_step[txl]: ", "emo_grammar_step[acc]: ", "emo_grammar_step[acc_window]: ", "emo_grammar_step[txl_queue]: ",
 * "emo_grammar_step[acc_queue]: ". */
int emo_grammar_step(const emo_grammar_step_t* args, emo_stream_t stream);
/* Re-anchor the streams that filled the window on a bar (no reference counterpart past the window: the reference slides the window token by token,
 * stage2_accompaniment/inference.py:252-257; this is the context its dataloader builds, dataloader.py:179-186: the piece's opening events followed by the
 * piece from a bar on, positions from 0).  One launch per phase, one 512-thread workgroup per row r of seq / segs (int64 [n_rows, ld_seq]), state / params
 * (int32 [n_rows, 8], the ACC layout) and primer_len (int32 [n_rows]: the row is primer_len[r] primer ids followed by bars that each open with
 * track_leadsheet).  For a row with state[STATUS] == EMO_ACC_WINDOW, n = state[LEN], P = primer_len[r]:
 *   b = the smallest i >= P with seq[i] == track_leadsheet and P + (n - i) <= keep; when no bar start fits, the last bar start, provided
 *       P + (n - b) <= window - longest_bar - 2; otherwise state[STATUS] = EMO_REBASE_BAR_TOO_LONG, new_len[r] = 0 and nothing else is written
 *       (inference.rebase_plan is the same rule on the host);
 *   dst_seq / dst_segs[r, 0 .. ld_dst) (int64 [n_rows, ld_dst], buffers other than seq / segs) = primer + seq / segs[b .. n), then pad / segment 1;
 *   the archive (arch_tok int64 [n_rows, ld_arch], arch_len int32 [n_rows], a cursor per row) takes seq[P .. b) at its cursor, which advances by b - P;
 *   with the score tables (tok_logp / tok_rank / tok_entropy [n_rows, ld_seq]; dst_* [n_rows, ld_dst]; arch_* [n_rows, ld_arch]: all nine or none) the
 *   same columns move with the tokens, and the destination cells behind the new length get the sentinels NaN / -1 / NaN;
 *   state: STATUS = RUNNING, LEN = CONSUMED = new_len = P + n - b, DRAWS = 0, the other words kept (bars, position, failed and accepted counts);
 *   params[MAX_EVENTS] -= b - P (the reference's whole-piece limit len(generated) > max_events, in the new row's indices); new_len[r] = the new
 *   length (int32 [n_rows]); *running (int32 [1]) += 1.
 * A row the archive or the destination cannot hold, or with a length outside its row, ends with EMO_ACC_OVERFLOW and new_len 0.  Any other row:
 * new_len[r] = 0 and nothing else is touched.  Requires 0 < keep <= window - longest_bar - 2 and window <= ld_dst.  Graph-capturable; nothing is allocated. */
typedef struct {
    int64_t n_rows;            /* workgroups launched: the rows of every table below */
    const int64_t* seq;        /* int64 [n_rows, ld_seq]: the rows as the last phase left them (never written) */
    const int64_t* segs;       /* int64 [n_rows, ld_seq] */
    int64_t ld_seq;
    int32_t* state;            /* int32 [n_rows, 8], the ACC layout: read, and rewritten for the rows that go on or end here */
    int32_t* params;           /* int32 [n_rows, 8]: MAX_EVENTS is lowered by the tokens dropped */
    const int32_t* primer_len; /* int32 [n_rows] */
    int64_t track_leadsheet, keep, window, longest_bar, pad;   /* 0 < keep <= window - longest_bar - 2 */
    int64_t* dst_seq;          /* int64 [n_rows, ld_dst], ld_dst >= window: the new contexts */
    int64_t* dst_segs;         /* int64 [n_rows, ld_dst] */
    int64_t ld_dst;
    int64_t* arch_tok;         /* int64 [n_rows, ld_arch]: the dropped tokens of every row, in order */
    int32_t* arch_len;         /* int32 [n_rows]: the archive cursors */
    int64_t ld_arch;
    /* the score tables of emo_grammar_step_t, all nine or none (NULL) */
    const float* tok_logp;     /* f32 [n_rows, ld_seq] */
    const int32_t* tok_rank;   /* int32 [n_rows, ld_seq] */
    const float* tok_entropy;  /* f32 [n_rows, ld_seq] */
    float* dst_logp;           /* f32 [n_rows, ld_dst] */
    int32_t* dst_rank;         /* int32 [n_rows, ld_dst] */
    float* dst_entropy;        /* f32 [n_rows, ld_dst] */
    float* arch_logp;          /* f32 [n_rows, ld_arch] */
    int32_t* arch_rank;        /* int32 [n_rows, ld_arch] */
    float* arch_entropy;       /* f32 [n_rows, ld_arch] */
    int32_t* new_len;          /* int32 [n_rows]: written for every row */
    int32_t* running;          /* int32 [1]: += 1 per row that goes on */
} emo_acc_rebase_t;
/* sizeof(emo_acc_rebase_t) as the library was built (a binding checks its mirror against it, as with emo_grammar_step_size) */
int emo_acc_rebase_size(void);
/* The block is read at call time, as emo_grammar_step_t is. */
int emo_acc_rebase(const emo_acc_rebase_t* args, emo_stream_t stream);
/* counts[0..5] += {nonpad, nonpad&correct, chord, chord&correct, melody, melody&correct} (train.py:184-193) */
int emo_accuracy_counts(const float* logits, const int64_t* tgt, const int64_t* chord,
                        const int64_t* melody, int64_t M, int64_t V, int64_t pad, int64_t* counts,
                        emo_stream_t stream);

/* ------------------------------------------------------------------ optimizer plumbing (K11, SURVEY f-3)
 * sumsq: acc[0] = sum x^2, bitwise reproducible (fixed summation order); acc = EMO_SUMSQ_FLOATS floats of caller scratch, zeroed once
 * before the first call (acc[1..1024] block partials, acc[1025] a ticket word the kernel returns to zero).  clip_coef: coef[0] = min(1, max_norm/(sqrt(sumsq*pre*pre)+1e-6)) * pre
 * (pre = 1/world for DP-averaged grads).  adam: torch.optim.Adam semantics (no amsgrad, wd=0),
 * grads scaled by gscale[0]; optionally refreshes the bf16 compute copy of the weights. */
#define EMO_SUMSQ_FLOATS 1026
int emo_sumsq(const float* x, int64_t n, float* acc, emo_stream_t stream);
/* coef = pre' * min(1, max_norm / (sqrt(sumsq) * pre' + 1e-6)) with pre' = pre / denom[0] (denom NULL => 1): the clip of
 * torch.nn.utils.clip_grad_norm_ (train.py:79) applied to the pre-scaled gradient.  Data parallel: pre = 1/world for equal
 * token counts, or pre = 1 and denom = the all-reduced number of non-pad target tokens (token-weighted global mean). */
int emo_clip_coef(const float* sumsq, float max_norm, float pre, const float* denom, float* coef, emo_stream_t stream);
int emo_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                  float beta1, float beta2, float eps, int64_t step, const float* gscale,
                  emo_stream_t stream);
int emo_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, emo_stream_t stream);
/* o1 = x + b1, o2 = x + b2 with per-column fp32 biases [D]; x [M, D] (row pitch ld), o1 / o2 contiguous [M, D], same dtype.  The biased
 * query copies qu = q + r_w_bias, qv = q + r_r_bias of the relative-position attention (stage1_compose/model/optimus_txl_decoder.py:331-341:
 * rw_head_q / rr_head_q) for the BWD_KV / BWD_R passes of EMO_ATTN_RELPOS, in one launch. */
int emo_add_bias2(const void* x, int64_t ld, const float* b1, const float* b2, void* o1, void* o2, int dtype,
                  int64_t M, int64_t D, emo_stream_t stream);
/* n bf16 transposes in one launch (no reference counterpart: the transposed weight mirrors that let every dgrad run as a k-contiguous NT
 * product, refreshed after an optimizer step).  desc: DEVICE array of n records of six int64 {src pointer, dst pointer, rows, cols, index of
 * the record's first 64 x 64 tile, tiles per row = ceil(cols / 64)}; src is [rows, cols] row-major, dst [cols, rows]; total_tiles = sum over
 * records of ceil(rows / 64) * ceil(cols / 64); rows and the pointers must allow 16-B accesses (rows % 8 == 0, cols % 8 == 0 fast path). */
int emo_transpose_batch(const int64_t* desc, int n, int64_t total_tiles, emo_stream_t stream);
/* Stream fork / join without a host round trip through torch's Stream objects (no reference counterpart: the weight-gradient products of
 * a layer run on a second stream beside the dgrad chain at small token counts): `waiter` continues only after everything queued on `signaler`
 * so far.  Asynchronous; events are owned by the library (per calling thread). */
int emo_stream_wait(emo_stream_t waiter, emo_stream_t signaler);

/* ------------------------------------------------------------------ data-parallel exchange (RCCL over xGMI)
 * The reference trains on one GPU; the build shards the batch over one process per GPU and adds ONE exchange per optimizer
 * step between loss.backward() and clip_grad_norm_ (insertion point train.py:76-81): a sum all-reduce of the flat fp32
 * gradient buffer (+ the non-pad token count in its last slot), and one broadcast of parameters / omega at start-up.
 * RCCL is bound with dlopen at the first call (no link-time dependency).  One communicator per process, bound to the
 * CURRENT HIP device at emo_comm_init; all transfers are in place, asynchronous on `stream`.
 *   emo_comm_bind      : dlopen RCCL and resolve its symbols, nothing else (every rank can test locally that the plane is usable)
 *   emo_comm_unique_id : rank 0 creates the 128-byte rendezvous id; the caller ships it to the other ranks (any side channel)
 *   emo_comm_init      : collective over all ranks (ncclCommInitRank)
 *   emo_comm_allreduce : buf[i] = sum over ranks (dtype EMO_F32 / EMO_BF16 / EMO_I64)
 *   emo_comm_broadcast : buf <- root's buf
 *   emo_comm_world/rank: 0 / -1 before init
 */
int emo_comm_bind(void);
int emo_comm_unique_id(void* id128);
int emo_comm_init(const void* id128, int rank, int world);
int emo_comm_world(void);
int emo_comm_rank(void);
int emo_comm_allreduce(void* buf, int64_t count, int dtype, emo_stream_t stream);
int emo_comm_broadcast(void* buf, int64_t count, int dtype, int root, emo_stream_t stream);
int emo_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* EMO_HIP_H */
