// Sequence scoring: per-row cross-entropy terms of fp32 logits (negative log-probability, log-sum-exp, rank of the target, entropy of the
// predicted distribution) and the cross-entropy backward with a per-row upstream gradient.  What F.cross_entropy(reduction='none' / 'sum')
// needs (stage2_accompaniment/model/music_performer.py:72-81, music_gpt2.py:94-103 pass `reduction` straight through) and what a scoring
// pass over a finished sequence reports.
//
// Row layout and reduction order are those of xent_fwd_regs_kernel / xent_fwd_kernel (emo_elementwise.hip): one wave per row, lane l owns
// columns l, l + 64, l + 128, ...; the row maximum by wave_max, the per-lane sum of expf(l - max) in ascending column order, then wave_sum.
// lse[m] is therefore bit-identical to emo_xent_fwd's row_lse[m] on the same values, on both paths (the only difference is the row stride:
// `ld` here, V there).  No LDS, no atomics: every output is a plain per-row vector store.
#include "emo_common.h"

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Lane 0 writes the outputs of one row.  s = sum of exp(l - mx), w = sum of exp(l - mx) (l - mx), cnt = columns ranked in front of the target.
//   entropy = lse - sum_v p_v l_v = log s - w / s      (p_v = exp(l_v - mx) / s)
__device__ __forceinline__ void score_store(int64_t row, bool scored, float mx, float s, float w, int cnt, float lt, float* __restrict__ nll,
                                            float* __restrict__ lse, int* __restrict__ rank, float* __restrict__ entropy) {
    const float ls = logf(s);
    const float z = mx + ls;
    nll[row] = scored ? z - lt : 0.f;
    if (lse) lse[row] = z;
    if (rank) rank[row] = scored ? cnt : -1;
    if (entropy) entropy[row] = ls - w / s;
}

// exp(x - mx) (x - mx) with the limit 0 where the exponential underflows (x = -inf, or a pad-fill value, would give 0 * inf)
__device__ __forceinline__ float score_wterm(float e, float d) { return e > 0.f ? e * d : 0.f; }

// V <= 64 * NV: the row lives in registers, two rows in flight per wave (as xent_fwd_regs_kernel)
template <int NV>
__global__ __launch_bounds__(256) void token_scores_regs_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ tgt,
                                                                int64_t M, int64_t V, int64_t ignore, float* __restrict__ nll,
                                                                float* __restrict__ lse, int* __restrict__ rank, float* __restrict__ entropy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 2; r0 < M; r0 += nw * 2) {
        const int64_t r1 = r0 + 1 < M ? r0 + 1 : r0;
        const float* l0 = logits + r0 * ld;
        const float* l1 = logits + r1 * ld;
        float a[NV], b[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int64_t c = lane + 64 * i;
            a[i] = c < V ? l0[c] : -INFINITY;
            b[i] = c < V ? l1[c] : -INFINITY;
        }
        // targets: wave-uniform loads; a row is scored when its target is not ignore_index (the host has refused anything else outside [0, V);
        // the range test only keeps a stray id from indexing outside the row)
        const int64_t t0 = tgt[r0], t1 = tgt[r1];
        const bool in0 = t0 >= 0 && t0 < V, in1 = t1 >= 0 && t1 < V;
        const bool sc0 = t0 != ignore && in0, sc1 = t1 != ignore && in1;
        const float lt0 = in0 ? l0[t0] : INFINITY, lt1 = in1 ? l1[t1] : INFINITY;
        float ma = a[0], mb = b[0];
#pragma unroll
        for (int i = 1; i < NV; ++i) { ma = fmaxf(ma, a[i]); mb = fmaxf(mb, b[i]); }
        ma = wave_max(ma); mb = wave_max(mb);
        float sa = 0.f, sb = 0.f, wa = 0.f, wb = 0.f;
        int ca = 0, cb = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int64_t c = lane + 64 * i;
            if (c < V) {
                const float da = a[i] - ma, db = b[i] - mb;
                const float ea = expf(da), eb = expf(db);
                sa += ea; sb += eb;
                wa += score_wterm(ea, da); wb += score_wterm(eb, db);
                ca += (a[i] > lt0 || (a[i] == lt0 && c < t0)) ? 1 : 0;     // first max wins, as emo_argmax: ties count only in front of the target
                cb += (b[i] > lt1 || (b[i] == lt1 && c < t1)) ? 1 : 0;
            }
        }
        sa = wave_sum(sa); sb = wave_sum(sb);
        if (entropy) { wa = wave_sum(wa); wb = wave_sum(wb); }
        if (rank) { ca = wave_sum_i(ca); cb = wave_sum_i(cb); }
        if (lane == 0) {
            score_store(r0, sc0, ma, sa, wa, ca, lt0, nll, lse, rank, entropy);
            if (r0 + 1 < M) score_store(r1, sc1, mb, sb, wb, cb, lt1, nll, lse, rank, entropy);
        }
    }
}

// any V: one wave per row, two passes over the row (the second one hits the cache), as xent_fwd_kernel
__global__ __launch_bounds__(256) void token_scores_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ tgt, int64_t M,
                                                           int64_t V, int64_t ignore, float* __restrict__ nll, float* __restrict__ lse,
                                                           int* __restrict__ rank, float* __restrict__ entropy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
        const float* l = logits + row * ld;
        const int64_t t = tgt[row];
        const bool in = t >= 0 && t < V;
        const bool sc = t != ignore && in;
        const float lt = in ? l[t] : INFINITY;
        float mx = -INFINITY;
        for (int64_t c = lane; c < V; c += 64) mx = fmaxf(mx, l[c]);
        mx = wave_max(mx);
        float s = 0.f, w = 0.f;
        int cnt = 0;
        for (int64_t c = lane; c < V; c += 64) {
            const float x = l[c], d = x - mx;
            const float e = expf(d);
            s += e;
            w += score_wterm(e, d);
            cnt += (x > lt || (x == lt && c < t)) ? 1 : 0;
        }
        s = wave_sum(s);
        if (entropy) w = wave_sum(w);
        if (rank) cnt = wave_sum_i(cnt);
        if (lane == 0) score_store(row, sc, mx, s, w, cnt, lt, nll, lse, rank, entropy);
    }
}

extern "C" int emo_token_scores(const float* logits, int64_t ld, const int64_t* tgt, int64_t M, int64_t V, int64_t ignore_index, float* nll,
                                float* lse, int32_t* rank, float* entropy, emo_stream_t stream) {
    EMO_CHECK(logits && tgt && nll, "emo_token_scores: null pointer (logits, tgt and nll are required)");
    EMO_CHECK(M > 0 && V > 0 && ld >= V, "emo_token_scores: bad shape (M %lld, V %lld, ld %lld)", (long long)M, (long long)V, (long long)ld);
    hipStream_t st = (hipStream_t)stream;
    if (V <= 512) {
        int64_t blocks = cdiv64(M, 8);                      // 4 waves x 2 rows per block step
        if (blocks > 2048) blocks = 2048;
        if (V <= 384) hipLaunchKernelGGL(token_scores_regs_kernel<6>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, tgt, M, V, ignore_index, nll, lse, rank, entropy);
        else hipLaunchKernelGGL(token_scores_regs_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, tgt, M, V, ignore_index, nll, lse, rank, entropy);
        EMO_LAUNCH_CHECK();
        return EMO_OK;
    }
    int64_t blocks = cdiv64(M, 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(token_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, tgt, M, V, ignore_index, nll, lse, rank, entropy);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

// ------------------------------------------------------------------------------------------------ backward with a per-row gradient
// The arithmetic of xent_bwd_kernel with gscale[0] replaced by grow[row]: with a constant grow the two agree bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void xent_bwd_rows_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ tgt,
                                                            const float* __restrict__ row_lse, const float* __restrict__ grow, T* __restrict__ dl,
                                                            int64_t ld_out, int64_t M, int64_t V, int64_t ignore) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
        const int64_t t = tgt[row];
        const float lse = row_lse[row];
        const float keep = (t != ignore) ? grow[row] : 0.f;
        for (int64_t c = lane; c < ld_out; c += 64) {
            float v = 0.f;
            if (c < V) v = (expf(logits[row * ld + c] - lse) - (c == t ? 1.f : 0.f)) * keep;
            dl[row * ld_out + c] = from_f32<T>(v);
        }
    }
}
extern "C" int emo_xent_bwd_rows(const float* logits, int64_t ld, const int64_t* tgt, const float* row_lse, const float* grow, void* dlogits,
                                 int64_t ld_out, int dtype_out, int64_t M, int64_t V, int64_t ignore_index, emo_stream_t stream) {
    EMO_CHECK(logits && tgt && row_lse && grow && dlogits, "emo_xent_bwd_rows: null pointer");
    EMO_CHECK(M > 0 && V > 0 && ld >= V && ld_out >= V, "emo_xent_bwd_rows: bad shape (M %lld, V %lld, ld %lld, ld_out %lld)", (long long)M,
              (long long)V, (long long)ld, (long long)ld_out);
    EMO_CHECK(dtype_out == EMO_F32 || dtype_out == EMO_BF16, "emo_xent_bwd_rows: dtype_out must be fp32 or bf16");
    int64_t blocks = cdiv64(M, 4);
    if (blocks > 4096) blocks = 4096;
    hipStream_t st = (hipStream_t)stream;
    if (dtype_out == EMO_F32) hipLaunchKernelGGL(xent_bwd_rows_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, tgt, row_lse, grow, (float*)dlogits, ld_out, M, V, ignore_index);
    else hipLaunchKernelGGL(xent_bwd_rows_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, tgt, row_lse, grow, (bf16_t*)dlogits, ld_out, M, V, ignore_index);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
