// What the five kinds of emo_grammar_step (emo_stage1_gen.hip: TXL, TXL_QUEUE; emo_stage2_gen.hip: ACC, ACC_WINDOW, ACC_QUEUE and the entry) share besides the draw.
// Each kernel takes the caller's emo_grammar_step_t by value as its one parameter (a field is fetched from the kernel arguments where it is used,
// so the fields of the other kinds cost nothing) and runs as one 512-thread workgroup per row.
#pragma once
#include "emo_nucleus.h"
#include "emo_draw_scores.h"

// The opening of every kind: the stream's state and params words (n_st / n_pr of them) into LDS, one barrier.  Thread 0 alone touches the
// stream's state in memory afterwards: the other threads decide from this copy, so a write of thread 0 can never change the path (and the
// barrier count) of a thread that has not read yet.
__device__ __forceinline__ void emo_grammar_open(const int32_t* st, int n_st, const int32_t* pr, int n_pr, int32_t* sst, int32_t* spr, int tid) {
    if (tid < n_st) sst[tid] = st[tid];
    if (tid < n_pr) spr[tid] = pr[tid];
    __syncthreads();
}

// The optional per-token outputs (tok_logp / tok_rank / tok_entropy).  Launch arguments, so the test is uniform over the grid: with all three
// NULL a kernel takes the path it had before they existed.
__device__ __forceinline__ bool emo_grammar_wants_scores(const emo_grammar_step_t& a) { return a.tok_logp || a.tok_rank || a.tok_entropy; }

// The figures of the draw that was accepted and appended at seq[r, c] (the token `word`, drawn from the logits row lr), by all 512 threads of
// the stream's workgroup (EMO_DRAW_SCORES_BARRIERS barriers); `red`: EMO_DRAW_SCORES_WORDS words of LDS beside the nucleus scratch.
__device__ __forceinline__ void emo_grammar_score(const emo_grammar_step_t& a, const float* __restrict__ lr, int64_t r, int64_t c, int64_t word,
                                                  float* red, int tid) {
    float logp = 0.f, entropy = 0.f;
    int32_t rank = 0;
    emo_draw_scores(lr, a.n_token, word, red, tid, [] { __syncthreads(); }, logp, rank, entropy);
    if (tid == 0) emo_draw_scores_store(a.tok_logp, a.tok_rank, a.tok_entropy, r * a.ld_seq + c, logp, rank, entropy);
}

// Whether the block has any of the optional sampling controls (mask_of / bias_of alone are not read).  emo_grammar_step asks on the host and
// launches the kernel's <true> or <false> instance: without controls a launch runs the code it ran before they existed.
__host__ __device__ __forceinline__ bool emo_grammar_has_controls(const emo_grammar_step_t& a) {
    return a.tok_mask || a.temp_of || a.top_p_of || a.tok_bias || a.top_k_of || a.min_p_of;
}

// What the draw of stream r runs under (r: the index of its params row: a stream, a job, or rows[b]): its ban row (NULL: none), its
// temperature / top_p, its bias row (NULL: none) and the two cuts behind top-p (top_k <= 0, min_p <= 0: off).  CTL false: the block's two
// scalars, both cuts off, and the accessor of the draw folds to the plain load.  CTL true: temp_of / top_p_of / top_k_of / min_p_of where
// present, row mask_of[r] of tok_mask and row bias_of[r] of tok_bias; a value outside [0, n_masks) is no mask and one outside [0, n_biases)
// no bias, so nothing outside the tables is ever read.
struct emo_grammar_controls_t {
    const uint32_t* ban;
    float temp, top_p;
    const float* bias;
    int32_t top_k;
    float min_p;
};
template <bool CTL>
__device__ __forceinline__ emo_grammar_controls_t emo_grammar_controls(const emo_grammar_step_t& a, int64_t r) {
    emo_grammar_controls_t c{nullptr, a.temperature, a.top_p, nullptr, 0, 0.f};
    if constexpr (CTL) {
        if (a.tok_mask && a.mask_of) {
            const int64_t m = a.mask_of[r];
            if (m >= 0 && m < a.n_masks) c.ban = a.tok_mask + m * ((a.n_token + 31) >> 5);
        }
        if (a.temp_of) c.temp = a.temp_of[r];
        if (a.top_p_of) c.top_p = a.top_p_of[r];
        if (a.tok_bias && a.bias_of) {
            const int64_t m = a.bias_of[r];
            if (m >= 0 && m < a.n_biases) c.bias = a.tok_bias + m * a.n_token;
        }
        if (a.top_k_of) c.top_k = a.top_k_of[r];
        if (a.min_p_of) c.min_p = a.min_p_of[r];
    }
    return c;
}

// The launches of the TXL and TXL_QUEUE kinds (emo_stage1_gen.hip), for emo_grammar_step, which has checked the block.
int emo_txl_grammar_launch(const emo_grammar_step_t& a, emo_stream_t stream);
int emo_txl_queue_launch(const emo_grammar_step_t& a, emo_stream_t stream);
