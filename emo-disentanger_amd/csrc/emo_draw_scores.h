// What the model assigned to ONE token of ONE stream's logits row, by the 512 threads of the stream's workgroup: the figures of emo_token_scores
// (emo_score.hip, emo_hip.h K9b) taken inside the grammar launch, from the row the draw was made from — always at temperature 1, whatever
// temperature the draw used:
//   logp    = l[tok] - lse,  lse = mx + log sum_v exp(l_v - mx)
//   rank    = #{v : l[v] > l[tok]} + #{v < tok : l[v] == l[tok]}
//   entropy = lse - sum_v softmax(l)_v l_v = log s - w / s      (s = sum exp(l - mx), w = sum exp(l - mx) (l - mx))
// The arithmetic per column is that of emo_token_scores; the reduction order is not (8 waves of 64 lanes, two columns per thread, wave
// partials added in wave order), so the floats agree with emo_token_scores to rounding, not bit for bit.  Ranks are exact.
// LDS: EMO_DRAW_SCORES_WORDS words of the caller's, used for the cross-wave reductions only — nothing of the nucleus scratch (emo_nucleus.h)
// is read or written, so the sorted state a redraw needs is still there afterwards.
#pragma once
#include "emo_common.h"

constexpr int EMO_DRAW_SCORES_WORDS = 32;                      // 8 wave partials each of: max, s, w, count
constexpr int EMO_DRAW_SCORES_BARRIERS = 2;                    // sync() calls of emo_draw_scores (every path)

// tid in [0, 512), V <= 1024, 0 <= tok < V; `sync` = a barrier over exactly the calling threads.  The caller has a barrier between any earlier
// use of `red` and this call.  The three figures come back in thread 0 (other threads: undefined).
template <typename Sync>
__device__ __forceinline__ void emo_draw_scores(const float* __restrict__ l, int64_t V, int64_t tok, float* red, int tid, Sync sync, float& logp,
                                                int32_t& rank, float& entropy) {
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = tid, c1 = tid + 512;
    const float x0 = c0 < V ? l[c0] : -INFINITY, x1 = c1 < V ? l[c1] : -INFINITY;
    const float lt = l[tok];                                   // (one address for the whole workgroup)
    float mx = wave_max(fmaxf(x0, x1));
    if (lane == 0) red[wave] = mx;
    sync();
    mx = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
    float s = 0.f, w = 0.f, cnt = 0.f;                         // (a count of at most 1024 is exact in fp32)
    if (c0 < V) {
        const float d = x0 - mx, e = expf(d);
        s += e;
        w += e > 0.f ? e * d : 0.f;                            // exp(d) d with the limit 0 where the exponential underflows (score_wterm)
        cnt += (x0 > lt || (x0 == lt && c0 < tok)) ? 1.f : 0.f;
    }
    if (c1 < V) {
        const float d = x1 - mx, e = expf(d);
        s += e;
        w += e > 0.f ? e * d : 0.f;
        cnt += (x1 > lt || (x1 == lt && c1 < tok)) ? 1.f : 0.f;
    }
    s = wave_sum(s);
    w = wave_sum(w);
    cnt = wave_sum(cnt);
    if (lane == 0) {
        red[8 + wave] = s;
        red[16 + wave] = w;
        red[24 + wave] = cnt;
    }
    sync();
    if (tid == 0) {
        float st = 0.f, wt = 0.f, ct = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            st += red[8 + i];
            wt += red[16 + i];
            ct += red[24 + i];
        }
        const float ls = logf(st);
        logp = lt - (mx + ls);
        rank = (int32_t)ct;
        entropy = ls - wt / st;
    }
}

// Thread 0 stores the figures the caller asked for (a NULL table: not wanted) at cell `at` = r * ld_seq + c of the [streams, ld_seq] tables.
__device__ __forceinline__ void emo_draw_scores_store(float* tok_logp, int32_t* tok_rank, float* tok_entropy, int64_t at, float logp, int32_t rank,
                                                      float entropy) {
    if (tok_logp) tok_logp[at] = logp;
    if (tok_rank) tok_rank[at] = rank;
    if (tok_entropy) tok_entropy[at] = entropy;
}
