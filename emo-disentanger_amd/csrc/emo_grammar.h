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

// The launches of the TXL and TXL_QUEUE kinds (emo_stage1_gen.hip), for emo_grammar_step, which has checked the block.
int emo_txl_grammar_launch(const emo_grammar_step_t& a, emo_stream_t stream);
int emo_txl_queue_launch(const emo_grammar_step_t& a, emo_stream_t stream);
