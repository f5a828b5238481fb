// Everything that walks fp32 logits rows: the cross-entropy of training (K9: per-row log-sum-exp, loss sum and count, backward), the
// per-row terms a scoring pass reports and F.cross_entropy(reduction='none' / 'sum') needs (K9b: negative log-probability, log-sum-exp, rank of
// the target, entropy of the predicted distribution; stage2_accompaniment/model/music_performer.py:72-81, music_gpt2.py:94-103 pass `reduction`
// straight through), the accuracy counts (K12) and the argmax.
//
// The four forward entries are operations on the one row walker of emo_logit_rows.h: they share its views, its reductions and its kernel, so
// lse[m] of emo_token_scores and row_lse[m] of emo_xent_fwd are the same instructions on the same values (only the row stride differs: `ld`
// there, V here), and emo_accuracy_counts counts a hit exactly where emo_argmax returns the target.  The two backward entries launch one kernel.
#include "emo_logit_rows.h"

// What differs between the entries' dispatch, by history and not by design: the smallest M that takes the register kernels, and the rows per
// block their grid is sized by.  The grid groups the loss partials into atomics and sets how many waves the training step's launches occupy.
static const int64_t kXentRegsMinM = 1024, kAccuracyRegsMinM = 1024, kScoresRegsMinM = 0;
static const int64_t kXentRegsRows = 4, kAccuracyRegsRows = 4, kScoresRegsRows = 8;

// ------------------------------------------------------------------------------------------------ cross-entropy forward
// acc[0] += sum of lse - l[tgt] over the rows whose target is not `ignore`, acc[1] += their number: one pair of atomics per block
struct XentFwdOp {
    const int64_t* tgt;
    int64_t ignore;
    float *row_lse, *acc;
    struct State { float lsum, lcnt; };
    template <int R, class Row>
    __device__ __forceinline__ void rows(State& st, const Row (&r)[R], const int64_t (&row)[R], int live, int64_t V, int lane) const {
        float mx[R], s[R];
        rows_max(r, V, lane, mx);
        rows_expsum(r, V, lane, mx, s, [](int64_t, const float (&)[R], const float (&)[R], const float (&)[R]) {});
        if (lane != 0) return;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k < live) {
                const float lse = mx[k] + logf(s[k]);
                row_lse[row[k]] = lse;
                const int64_t t = tgt[row[k]];
                if (t != ignore) { st.lsum += lse - r[k].global(t); st.lcnt += 1.f; }
            }
    }
    __device__ __forceinline__ void finish(const State& st, int lane, int wave) const {
        __shared__ float part[2][4];
        if (lane == 0) { part[0][wave] = st.lsum; part[1][wave] = st.lcnt; }
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd(acc, part[0][0] + part[0][1] + part[0][2] + part[0][3]);
            atomicAdd(acc + 1, part[1][0] + part[1][1] + part[1][2] + part[1][3]);
        }
    }
};
extern "C" int emo_xent_fwd(const float* logits, const int64_t* tgt, int64_t M, int64_t V, int64_t ignore_index, float* row_lse,
                            float* acc, emo_stream_t stream) {
    EMO_CHECK(logits && tgt && row_lse && acc, "emo_xent_fwd: null pointer");
    launch_logit_rows(XentFwdOp{tgt, ignore_index, row_lse, acc}, logits, V, M, V, kXentRegsMinM, kXentRegsRows, (hipStream_t)stream);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

// ------------------------------------------------------------------------------------------------ per-row scores
// No LDS, no atomics: every output is a plain per-row vector store.
struct TokenScoresOp {
    const int64_t* tgt;
    int64_t ignore;
    float *nll, *lse;
    int* rank;
    float* entropy;
    struct State {};
    template <int R, class Row>
    __device__ __forceinline__ void rows(State&, const Row (&r)[R], const int64_t (&row)[R], int live, int64_t V, int lane) const {
        // targets: wave-uniform loads; a row is scored when its target is not ignore_index (the host has refused anything else outside [0, V);
        // the range test only keeps a stray id from indexing outside the row)
        int64_t t[R];
        bool sc[R];
        float lt[R], mx[R], s[R], w[R];
        int cnt[R];
#pragma unroll
        for (int k = 0; k < R; ++k) t[k] = tgt[row[k]];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const bool in = t[k] >= 0 && t[k] < V;
            sc[k] = t[k] != ignore && in;
            lt[k] = in ? r[k].global(t[k]) : INFINITY;
            w[k] = 0.f;
            cnt[k] = 0;
        }
        rows_max(r, V, lane, mx);
        rows_expsum(r, V, lane, mx, s, [&](int64_t c, const float (&x)[R], const float (&d)[R], const float (&e)[R]) {
#pragma unroll
            for (int k = 0; k < R; ++k) w[k] += score_wterm(e[k], d[k]);
#pragma unroll
            for (int k = 0; k < R; ++k) cnt[k] += (x[k] > lt[k] || (x[k] == lt[k] && c < t[k])) ? 1 : 0;      // first max wins, as rows_argmax: ties count only in front of the target
        });
        if (entropy) {
#pragma unroll
            for (int k = 0; k < R; ++k) w[k] = wave_sum(w[k]);
        }
        if (rank) {
#pragma unroll
            for (int k = 0; k < R; ++k) cnt[k] = wave_sum_i(cnt[k]);
        }
        if (lane != 0) return;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k < live) score_store(row[k], sc[k], mx[k], s[k], w[k], cnt[k], lt[k], nll, lse, rank, entropy);
    }
    __device__ __forceinline__ void finish(const State&, int, int) const {}
};
extern "C" int emo_token_scores(const float* logits, int64_t ld, const int64_t* tgt, int64_t M, int64_t V, int64_t ignore_index, float* nll,
                                float* lse, int32_t* rank, float* entropy, emo_stream_t stream) {
    EMO_CHECK(logits && tgt && nll, "emo_token_scores: null pointer (logits, tgt and nll are required)");
    EMO_CHECK(M > 0 && V > 0 && ld >= V, "emo_token_scores: bad shape (M %lld, V %lld, ld %lld)", (long long)M, (long long)V, (long long)ld);
    launch_logit_rows(TokenScoresOp{tgt, ignore_index, nll, lse, rank, entropy}, logits, ld, M, V, kScoresRegsMinM, kScoresRegsRows,
                      (hipStream_t)stream);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

// ------------------------------------------------------------------------------------------------ argmax / accuracy counts
struct ArgmaxOp {
    int64_t* out;
    struct State {};
    template <int R, class Row>
    __device__ __forceinline__ void rows(State&, const Row (&r)[R], const int64_t (&row)[R], int live, int64_t V, int lane) const {
        int64_t bi[R];
        rows_argmax(r, V, lane, bi);
        if (lane != 0) return;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k < live) out[row[k]] = bi[k];
    }
    __device__ __forceinline__ void finish(const State&, int, int) const {}
};
// one row per wave on a grid that covers the rows (the decode loops call this with a handful of rows)
extern "C" int emo_argmax(const float* logits, int64_t rows, int64_t V, int64_t* out, emo_stream_t stream) {
    EMO_CHECK(logits && out && rows > 0 && V > 0, "emo_argmax: bad args");
    hipLaunchKernelGGL((logit_rows_kernel<0, ArgmaxOp>), dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, (hipStream_t)stream, logits, V, rows, V,
                       ArgmaxOp{out});
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

// counts[0..5] += rows with tgt != pad, hits among them, chord rows, hits, melody rows, hits
struct AccuracyOp {
    const int64_t *tgt, *chord, *melody;
    int64_t pad;
    unsigned long long* counts;
    struct State { unsigned long long c[6]; };
    template <int R, class Row>
    __device__ __forceinline__ void rows(State& st, const Row (&r)[R], const int64_t (&row)[R], int live, int64_t V, int lane) const {
        int64_t bi[R];
        rows_argmax(r, V, lane, bi);
        if (lane != 0) return;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k < live) {
                const int64_t t = tgt[row[k]];
                const unsigned long long ok = (bi[k] == t);
                if (t != pad) { st.c[0]++; st.c[1] += ok; }
                if (chord && chord[row[k]] == 1) { st.c[2]++; st.c[3] += ok; }
                if (melody && melody[row[k]] == 1) { st.c[4]++; st.c[5] += ok; }
            }
    }
    __device__ __forceinline__ void finish(const State& st, int lane, int) const {
        if (lane == 0)
            for (int i = 0; i < 6; ++i)
                if (st.c[i]) atomicAdd(counts + i, st.c[i]);
    }
};
extern "C" int emo_accuracy_counts(const float* logits, const int64_t* tgt, const int64_t* chord, const int64_t* melody, int64_t M,
                                   int64_t V, int64_t pad, int64_t* counts, emo_stream_t stream) {
    EMO_CHECK(logits && tgt && counts, "emo_accuracy_counts: null pointer");
    launch_logit_rows(AccuracyOp{tgt, chord, melody, pad, (unsigned long long*)counts}, logits, V, M, V, kAccuracyRegsMinM, kAccuracyRegsRows,
                      (hipStream_t)stream);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

// ------------------------------------------------------------------------------------------------ cross-entropy backward
// dl[m, c] = (exp(l[m, c] - lse[m]) - [c == tgt[m]]) g for c < V on the rows whose target is not `ignore`, 0 elsewhere and in the columns
// V .. ld_out.  g is grad[0], the scalar upstream gradient of the mean loss, or with kRowGrad grad[m]: with a constant one the two agree bit for bit.
template <typename T, bool kRowGrad>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ tgt,
                                                       const float* __restrict__ row_lse, const float* __restrict__ grad, T* __restrict__ dl,
                                                       int64_t ld_out, int64_t M, int64_t V, int64_t ignore) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float gs = kRowGrad ? 0.f : grad[0];
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
        const int64_t t = tgt[row];
        const float lse = row_lse[row];
        const float keep = (t != ignore) ? (kRowGrad ? grad[row] : gs) : 0.f;
        for (int64_t c = lane; c < ld_out; c += 64) {
            float v = 0.f;
            if (c < V) v = (expf(logits[row * ld + c] - lse) - (c == t ? 1.f : 0.f)) * keep;
            dl[row * ld_out + c] = from_f32<T>(v);
        }
    }
}
template <bool kRowGrad>
static void launch_xent_bwd(const float* logits, int64_t ld, const int64_t* tgt, const float* row_lse, const float* grad, void* dlogits,
                            int64_t ld_out, int dtype_out, int64_t M, int64_t V, int64_t ignore, hipStream_t st) {
    int64_t blocks = cdiv64(M, 4);
    if (blocks > 4096) blocks = 4096;
    if (dtype_out == EMO_F32) hipLaunchKernelGGL((xent_bwd_kernel<float, kRowGrad>), dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, tgt, row_lse, grad, (float*)dlogits, ld_out, M, V, ignore);
    else hipLaunchKernelGGL((xent_bwd_kernel<bf16_t, kRowGrad>), dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, tgt, row_lse, grad, (bf16_t*)dlogits, ld_out, M, V, ignore);
}
extern "C" int emo_xent_bwd(const float* logits, const int64_t* tgt, const float* row_lse, const float* gscale, void* dlogits,
                            int64_t ld_out, int dtype_out, int64_t M, int64_t V, int64_t ignore_index, emo_stream_t stream) {
    EMO_CHECK(logits && tgt && row_lse && gscale && dlogits && ld_out >= V, "emo_xent_bwd: bad args");
    launch_xent_bwd<false>(logits, V, tgt, row_lse, gscale, dlogits, ld_out, dtype_out, M, V, ignore_index, (hipStream_t)stream);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
extern "C" int emo_xent_bwd_rows(const float* logits, int64_t ld, const int64_t* tgt, const float* row_lse, const float* grow, void* dlogits,
                                 int64_t ld_out, int dtype_out, int64_t M, int64_t V, int64_t ignore_index, emo_stream_t stream) {
    EMO_CHECK(logits && tgt && row_lse && grow && dlogits, "emo_xent_bwd_rows: null pointer");
    EMO_CHECK(M > 0 && V > 0 && ld >= V && ld_out >= V, "emo_xent_bwd_rows: bad shape (M %lld, V %lld, ld %lld, ld_out %lld)", (long long)M,
              (long long)V, (long long)ld, (long long)ld_out);
    EMO_CHECK(dtype_out == EMO_F32 || dtype_out == EMO_BF16, "emo_xent_bwd_rows: dtype_out must be fp32 or bf16");
    launch_xent_bwd<true>(logits, ld, tgt, row_lse, grow, dlogits, ld_out, dtype_out, M, V, ignore_index, (hipStream_t)stream);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
