// Walking fp32 logits rows, device side: the one layout and the one set of per-row reductions behind emo_xent_fwd, emo_token_scores,
// emo_accuracy_counts and emo_argmax (emo_score.hip).  A wave owns a row; lane l owns columns l, l + 64, l + 128, ...; a row is reduced by
// wave_max / wave_sum / wave_argmax and lane 0 writes its outputs.  Because every entry runs THIS code, two entries agree bit for bit on
// whatever they both compute (the log-sum-exp of emo_xent_fwd and emo_token_scores; argmax == target exactly where rank == 0), on either
// view and at any row stride.
#pragma once
#include "emo_common.h"

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the larger value, the lower index among equal values
__device__ __forceinline__ void wave_argmax(float& v, int64_t& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(v, o, 64);
        int64_t oi = __shfl_xor(idx, o, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

// ------------------------------------------------------------------------------------------------ row views
// each(V, lane, f) calls f(c, i) for the lane's columns c = lane + 64 i < V in ascending order; at(c, i) is the value there and global(c) reads
// any column of the row from memory (the target's, which another lane owns).  The reductions below take R rows at once and visit a column
// of all of them in one step, so the arithmetic of two rows in flight interleaves.
// Register view, V <= 64 NV: the row is read once; a column at or beyond V holds -inf.
template <int NV>
struct RegRow {
    const float* l;
    float v[NV];
    // R rows at once, column group by column group: the loads of all rows are in flight before any is used, and come back in the order the
    // reductions consume them
    template <int R>
    static __device__ __forceinline__ void load(RegRow (&r)[R], const float* logits, int64_t ld, const int64_t (&row)[R], int64_t V, int lane) {
#pragma unroll
        for (int k = 0; k < R; ++k) r[k].l = logits + row[k] * ld;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int64_t c = lane + 64 * i;
#pragma unroll
            for (int k = 0; k < R; ++k) r[k].v[i] = c < V ? r[k].l[c] : -INFINITY;
        }
    }
    template <class F>
    static __device__ __forceinline__ void each(int64_t V, int lane, F&& f) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int64_t c = lane + 64 * i;
            if (c < V) f(c, i);
        }
    }
    // every register, the -inf ones included: for a reduction that -inf does not change, without a bounds test per column
    template <class F>
    static __device__ __forceinline__ void each_padded(int64_t, int lane, F&& f) {
#pragma unroll
        for (int i = 0; i < NV; ++i) f(lane + 64 * i, i);
    }
    __device__ __forceinline__ float at(int64_t, int i) const { return v[i]; }
    __device__ __forceinline__ float global(int64_t c) const { return l[c]; }
};
// Memory view, any V: every pass reads the row again (the second one hits the cache).
struct MemRow {
    const float* l;
    template <class F>
    static __device__ __forceinline__ void each(int64_t V, int lane, F&& f) {
        for (int64_t c = lane; c < V; c += 64) f(c, 0);
    }
    template <class F>
    static __device__ __forceinline__ void each_padded(int64_t V, int lane, F&& f) { each(V, lane, f); }
    __device__ __forceinline__ float at(int64_t c, int) const { return l[c]; }
    __device__ __forceinline__ float global(int64_t c) const { return l[c]; }
};

// ------------------------------------------------------------------------------------------------ per-row reductions, result in every lane
template <int R, class Row>
__device__ __forceinline__ void rows_max(const Row (&r)[R], int64_t V, int lane, float (&mx)[R]) {
#pragma unroll
    for (int k = 0; k < R; ++k) mx[k] = -INFINITY;
    Row::each_padded(V, lane, [&](int64_t c, int i) {
#pragma unroll
        for (int k = 0; k < R; ++k) mx[k] = fmaxf(mx[k], r[k].at(c, i));
    });
#pragma unroll
    for (int k = 0; k < R; ++k) mx[k] = wave_max(mx[k]);
}

// s = sum of expf(x - mx): per lane in ascending column order, then wave_sum.  term(c, x, d, e) sees every column c with the R rows' values
// x[k], d[k] = x[k] - mx[k] and e[k] = expf(d[k]), for what an entry sums besides.  One quantity at a time over the rows: in this order the
// compiler pairs the two rows' arithmetic into packed instructions.
template <int R, class Row, class F>
__device__ __forceinline__ void rows_expsum(const Row (&r)[R], int64_t V, int lane, const float (&mx)[R], float (&s)[R], F&& term) {
#pragma unroll
    for (int k = 0; k < R; ++k) s[k] = 0.f;
    Row::each(V, lane, [&](int64_t c, int i) {
        float x[R], d[R], e[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            x[k] = r[k].at(c, i);
            d[k] = x[k] - mx[k];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) e[k] = expf(d[k]);
#pragma unroll
        for (int k = 0; k < R; ++k) s[k] += e[k];
        term(c, x, d, e);
    });
#pragma unroll
    for (int k = 0; k < R; ++k) s[k] = wave_sum(s[k]);
}

// The lowest index among the row's maxima, as numpy / torch argmax.  Inside a lane the first maximum wins (ascending column) and a NaN is taken
// only while the lane has nothing yet; a row of -inf only beats the start value nowhere and gets index 0.
template <int R, class Row>
__device__ __forceinline__ void rows_argmax(const Row (&r)[R], int64_t V, int lane, int64_t (&bi)[R]) {
    float best[R];
    int64_t idx[R];
#pragma unroll
    for (int k = 0; k < R; ++k) { best[k] = -INFINITY; idx[k] = INT64_MAX; }
    Row::each(V, lane, [&](int64_t c, int i) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const float x = r[k].at(c, i);
            if (x > best[k] || (x != x && idx[k] == INT64_MAX)) { best[k] = x; idx[k] = c; }
        }
    });
#pragma unroll
    for (int k = 0; k < R; ++k) wave_argmax(best[k], idx[k]);
#pragma unroll
    for (int k = 0; k < R; ++k) bi[k] = idx[k] == INT64_MAX ? 0 : idx[k];
}

// exp(x - mx) (x - mx) with the limit 0 where the exponential underflows (x = -inf, or a pad-fill value, would give 0 * inf)
__device__ __forceinline__ float score_wterm(float e, float d) { return e > 0.f ? e * d : 0.f; }

// Lane 0 writes the scores of one row.  s = sum of exp(l - mx), w = sum of exp(l - mx) (l - mx), cnt = columns ranked in front of the target.
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

// ------------------------------------------------------------------------------------------------ the kernel
// An operation Op has a per-lane State, rows(st, r, row, live, V, lane) for R rows at once (views r[k] of rows row[k]; only k < live may be
// written or counted) and finish(st, lane, wave) at the end of the block.
//   NV == 0: one row per wave over a MemRow.
//   NV > 0:  two RegRows per wave step, both loaded before either is reduced; an odd last row is walked twice and emitted once.
template <int NV, class Op>
__global__ __launch_bounds__(256) void logit_rows_kernel(const float* __restrict__ logits, int64_t ld, int64_t M, int64_t V, Op op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nw = (int64_t)gridDim.x * 4;
    typename Op::State st{};
    if constexpr (NV == 0) {
        for (int64_t r0 = (int64_t)blockIdx.x * 4 + wave; r0 < M; r0 += nw) {
            const MemRow r[1] = {{logits + r0 * ld}};
            const int64_t row[1] = {r0};
            op.rows(st, r, row, 1, V, lane);
        }
    } else {
        for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 2; r0 < M; r0 += nw * 2) {
            const int64_t row[2] = {r0, r0 + 1 < M ? r0 + 1 : r0};
            RegRow<NV> r[2];
            RegRow<NV>::load(r, logits, ld, row, V, lane);
            op.rows(st, r, row, r0 + 1 < M ? 2 : 1, V, lane);
        }
    }
    op.finish(st, lane, wave);
}

// Where an entry's rows go: V <= 384 and V <= 512 to the register kernels once M reaches regs_min_m, on a grid of one block per regs_rows
// rows; everything else to the memory kernel on one block per 4 rows.  Both grids are capped at 2048 blocks and stride.
template <class Op>
static void launch_logit_rows(const Op& op, const float* logits, int64_t ld, int64_t M, int64_t V, int64_t regs_min_m, int64_t regs_rows,
                              hipStream_t st) {
    const bool regs = V <= 512 && M >= regs_min_m;
    int64_t blocks = cdiv64(M, regs ? regs_rows : 4);
    if (blocks > 2048) blocks = 2048;
    if (!regs) hipLaunchKernelGGL((logit_rows_kernel<0, Op>), dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, M, V, op);
    else if (V <= 384) hipLaunchKernelGGL((logit_rows_kernel<6, Op>), dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, M, V, op);
    else hipLaunchKernelGGL((logit_rows_kernel<8, Op>), dim3((unsigned)blocks), dim3(256), 0, st, logits, ld, M, V, op);
}
