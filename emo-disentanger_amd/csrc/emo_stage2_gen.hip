// Stage-2 accompaniment generation: the sample-and-grammar half of one lock-step token step (reference stage2_accompaniment/inference.py
// generate_conditional :231-327, as restated by inference._Stream.offer and generate_conditional_batch's loop body).  One 512-thread workgroup
// per stream; all loop state lives in device memory (no allocation, graph-capturable).  The draw is emo_nucleus_draw, the device code of
// emo_sample_nucleus, so a stream picks the same id from the same logits and uniform.
// Per stream r:
//   finished                    -> tok_out[r] = pad, seg_out[r] = 1;
//   len >= max_len              -> WINDOW (the host hands the stream to the full-window loop), fed like a finished stream;
//   tokens not yet fed          -> tok_out[r] = seq[r, consumed] (a primer longer than the common prefix, the sampled word, an injected bar);
//   otherwise                   -> draw, grammar; a rejection draws again from the same logits with the next uniform (the reference's
//                                  `continue`; emo_nucleus_pick reuses the sorted probabilities), so a stream advances exactly one token
//                                  per step; after an acceptance the new token is fed.
// emo_acc_window_step is the same draw and grammar (acc_draw below, shared) for streams past the window (reference :252-277: the model input is
// the last max_dec_inp_len tokens, positions restarting at 0): nothing is fed token by token; after an acceptance the stream's next model input
// win_tok / win_seg[b, 0..W) = seq / segs[r, LEN - W .. LEN) is written, an injected bar included.
#include "emo_nucleus.h"

namespace {

// The draws of one launch of one stream, shared by the in-window and the windowed step: draw until the grammar accepts or ends the stream.
// `draws` advances in every thread alike, and thread 0 runs the grammar on the LDS copy of the state (kept there, not in registers, across the
// draws); it alone gets the status back (the other threads: RUNNING).  u_col: the stream's column of the uniform table, pitch ld_u.
__device__ __forceinline__ int32_t acc_draw(const float* __restrict__ lr, int64_t V, float temp, float top_p, const float* __restrict__ u_col,
                                            int64_t ld_u, int64_t n_u, const int32_t* __restrict__ ev_flags, const int32_t* __restrict__ ev_beat,
                                            const int64_t* __restrict__ lead_tok, const int32_t* __restrict__ lead_off, const int32_t* spr, int32_t* sst,
                                            int32_t* sagain_p, int64_t* __restrict__ row, int64_t* __restrict__ srow, int64_t ld_seq, int64_t track_full,
                                            char* lds, int tid, int32_t& draws) {
    int32_t& sagain = *sagain_p;
    int32_t status = EMO_ACC_RUNNING;
    const int32_t draws0 = draws;
    for (;;) {
        if (draws >= n_u) {                                  // the caller's uniform table is exhausted: never read past it
            status = EMO_ACC_OUT_OF_DRAWS;
            break;
        }
        // a redraw from the same logits needs only the cut and the pick over the sorted state the first draw left in LDS (the same operations
        // on the same data: the id a fresh emo_nucleus_draw with this uniform would give)
        const float u = u_col[(int64_t)draws * ld_u];
        const int64_t word = draws == draws0 ? emo_nucleus_draw(lr, V, temp, top_p, u, lds, tid, [] { __syncthreads(); })
                                            : emo_nucleus_pick(V, top_p, u, lds, tid, [] { __syncthreads(); });
        ++draws;
        if (tid == 0) {
            const int32_t fl = ev_flags[word], target = spr[EMO_ACC_P_TARGET_BARS], bars = sst[EMO_ACC_S_BARS];
            int32_t len = sst[EMO_ACC_S_LEN];
            bool reject = false;
            if (spr[EMO_ACC_P_SKIP_CHECK] == 0 && (fl & EMO_ACC_EV_BEAT)) {   // Beat positions never go back inside a bar
                const int32_t pos = ev_beat[word];
                if (pos < sst[EMO_ACC_S_CUR_POS]) {
                    if (++sst[EMO_ACC_S_FAILED] >= 256) status = EMO_ACC_STUCK;  // the reference returns `generated` as it is
                    else reject = true;
                } else {
                    sst[EMO_ACC_S_CUR_POS] = pos;
                    sst[EMO_ACC_S_FAILED] = 0;
                }
            }
            if (status == EMO_ACC_RUNNING && !reject) {
                if (fl & EMO_ACC_EV_TRACK_LS) {              // the bar is done: inject the next lead-sheet bar, or finish
                    const bool more = bars + 1 < target;
                    const bool have = more && bars + 1 < spr[EMO_ACC_P_N_BARS];
                    const int32_t j = spr[EMO_ACC_P_BAR0] + bars + 1;
                    const int32_t a = have ? lead_off[j] : 0, b = have ? lead_off[j + 1] : 0;
                    if ((more && (!have || b < a)) || len + 1 + (more ? b - a + 1 : 0) > ld_seq) {
                        status = EMO_ACC_OVERFLOW;
                    } else {
                        row[len] = word;
                        srow[len++] = 0;
                        sst[EMO_ACC_S_BARS] = bars + 1;
                        ++sst[EMO_ACC_S_ACCEPTED];
                        if (more) {
                            for (int32_t i = a; i < b; ++i) {
                                row[len] = lead_tok[i];
                                srow[len++] = 0;
                            }
                            row[len] = track_full;
                            srow[len++] = 1;
                            sst[EMO_ACC_S_CUR_POS] = 0;
                        } else {
                            status = EMO_ACC_DONE;
                        }
                    }
                } else if ((fl & EMO_ACC_EV_PAD) || ((fl & EMO_ACC_EV_EOS) && bars < target - 1)) {
                    reject = true;                           // not counted toward failed_cnt
                } else if (len + 1 > ld_seq) {
                    status = EMO_ACC_OVERFLOW;
                } else {
                    row[len] = word;
                    srow[len++] = 1;
                    ++sst[EMO_ACC_S_ACCEPTED];
                    if (((fl & EMO_ACC_EV_EOS) && bars == target - 1) || len > spr[EMO_ACC_P_MAX_EVENTS]) status = EMO_ACC_DONE;
                }
            }
            sst[EMO_ACC_S_LEN] = len;
            sagain = (status == EMO_ACC_RUNNING && reject) ? 1 : 0;
        }
        __syncthreads();
        // (sagain is rewritten only after the next draw's barriers, which every thread reaches after this read)
        if (!sagain) break;
    }
    return status;
}

__global__ __launch_bounds__(512) void acc_grammar_kernel(const float* __restrict__ logits, int64_t n, int64_t V, float temp, float top_p,
                                                          const float* __restrict__ u_steps, int64_t n_u, const int32_t* __restrict__ ev_flags,
                                                          const int32_t* __restrict__ ev_beat, const int64_t* __restrict__ lead_tok,
                                                          const int32_t* __restrict__ lead_off, const int32_t* __restrict__ params,
                                                          int32_t* __restrict__ state, int64_t* __restrict__ seq, int64_t* __restrict__ segs,
                                                          int64_t ld_seq, int64_t max_len, int64_t track_full, int64_t pad,
                                                          int64_t* __restrict__ tok_out, int64_t* __restrict__ seg_out, int32_t* __restrict__ running) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_ACC_STATE_WORDS], spr[EMO_ACC_PARAM_WORDS], sagain;
    const int tid = (int)threadIdx.x;
    const int64_t r = blockIdx.x;
    int32_t* st = state + r * EMO_ACC_STATE_WORDS;
    int64_t* row = seq + r * ld_seq;
    int64_t* srow = segs + r * ld_seq;
    // thread 0 alone touches the stream's state in memory: the other threads decide from this copy, so a write below can never change the
    // path (and the barrier count) of a thread that has not read yet
    if (tid < EMO_ACC_STATE_WORDS) sst[tid] = st[tid];
    if (tid < EMO_ACC_PARAM_WORDS) spr[tid] = params[r * EMO_ACC_PARAM_WORDS + tid];
    __syncthreads();
    if (sst[EMO_ACC_S_STATUS] != EMO_ACC_RUNNING) {
        if (tid == 0) {
            tok_out[r] = pad;
            seg_out[r] = 1;
        }
        return;
    }
    if (sst[EMO_ACC_S_LEN] >= max_len) {                     // checked before the feed test, like the host loop's `overflow`
        if (tid == 0) {
            st[EMO_ACC_S_STATUS] = EMO_ACC_WINDOW;
            atomicSub(running, 1);
            tok_out[r] = pad;
            seg_out[r] = 1;
        }
        return;
    }
    int32_t consumed = sst[EMO_ACC_S_CONSUMED];
    if (consumed < sst[EMO_ACC_S_LEN]) {
        if (tid == 0) {
            tok_out[r] = row[consumed];
            seg_out[r] = srow[consumed];
            st[EMO_ACC_S_CONSUMED] = consumed + 1;
        }
        return;
    }
    int32_t draws = sst[EMO_ACC_S_DRAWS];
    const int32_t status = acc_draw(logits + r * V, V, temp, top_p, u_steps + r, n, n_u, ev_flags, ev_beat, lead_tok, lead_off, spr, sst, &sagain, row,
                                    srow, ld_seq, track_full, lds, tid, draws);
    if (tid != 0) return;
    if (status == EMO_ACC_RUNNING) {                         // the accepted word (or Track_LeadSheet before an injected bar) is the next input
        tok_out[r] = row[consumed];
        seg_out[r] = srow[consumed];
        ++consumed;
    } else {
        tok_out[r] = pad;
        seg_out[r] = 1;
        atomicSub(running, 1);
    }
    sst[EMO_ACC_S_STATUS] = status;
    sst[EMO_ACC_S_CONSUMED] = consumed;
    sst[EMO_ACC_S_DRAWS] = draws;
    for (int i = 0; i < EMO_ACC_STATE_WORDS; ++i) st[i] = sst[i];
}

__global__ __launch_bounds__(512) void acc_window_kernel(const float* __restrict__ logits, int64_t V, float temp, float top_p,
                                                         const float* __restrict__ u_steps, int64_t n_u, int64_t ld_u, const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ ev_flags, const int32_t* __restrict__ ev_beat,
                                                         const int64_t* __restrict__ lead_tok, const int32_t* __restrict__ lead_off,
                                                         const int32_t* __restrict__ params, int32_t* __restrict__ state, int64_t* seq, int64_t* segs,
                                                         int64_t ld_seq, int64_t W, int64_t track_full,
                                                         int64_t* __restrict__ win_tok, int64_t* __restrict__ win_seg, int32_t* __restrict__ running) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_ACC_STATE_WORDS], spr[EMO_ACC_PARAM_WORDS], sagain;
    const int tid = (int)threadIdx.x;
    const int64_t b = blockIdx.x;                            // row of the batch: logits, win_tok, win_seg
    const int64_t r = rows ? rows[b] : b;                    // the stream: state, params, seq, segs, column of u_steps
    if (r < 0 || r >= ld_u) return;                          // (not a stream of the table: nothing is read or written for it)
    int32_t* st = state + r * EMO_ACC_STATE_WORDS;
    int64_t* row = seq + r * ld_seq;
    int64_t* srow = segs + r * ld_seq;
    if (tid < EMO_ACC_STATE_WORDS) sst[tid] = st[tid];
    if (tid < EMO_ACC_PARAM_WORDS) spr[tid] = params[r * EMO_ACC_PARAM_WORDS + tid];
    __syncthreads();
    if (sst[EMO_ACC_S_STATUS] != EMO_ACC_RUNNING) return;    // finished: its window row stays as it is
    if (sst[EMO_ACC_S_LEN] < W || sst[EMO_ACC_S_LEN] > ld_seq) {   // no full window to read: a caller error, never a read outside the row
        if (tid == 0) {
            st[EMO_ACC_S_STATUS] = EMO_ACC_OVERFLOW;
            atomicSub(running, 1);
        }
        return;
    }
    int32_t draws = sst[EMO_ACC_S_DRAWS];
    const int32_t status = acc_draw(logits + b * V, V, temp, top_p, u_steps + r, ld_u, n_u, ev_flags, ev_beat, lead_tok, lead_off, spr, sst, &sagain, row,
                                    srow, ld_seq, track_full, lds, tid, draws);
    if (tid == 0) {
        if (status != EMO_ACC_RUNNING) atomicSub(running, 1);
        sst[EMO_ACC_S_STATUS] = status;
        sst[EMO_ACC_S_DRAWS] = draws;
        for (int i = 0; i < EMO_ACC_STATE_WORDS; ++i) st[i] = sst[i];
    }
    __syncthreads();                                         // thread 0's status, length and new tokens are visible to the workgroup
    if (sst[EMO_ACC_S_STATUS] != EMO_ACC_RUNNING) return;
    const int64_t off = (int64_t)sst[EMO_ACC_S_LEN] - W;     // >= 0: the length only grows
    for (int64_t i = tid; i < W; i += 512) {
        win_tok[b * W + i] = row[off + i];
        win_seg[b * W + i] = srow[off + i];
    }
}

}  // namespace

extern "C" int emo_acc_grammar_step(const float* logits, int64_t n, int64_t V, float temperature, float top_p, const float* u_steps, int64_t n_u,
                                    const int32_t* ev_flags, const int32_t* ev_beat, const int64_t* lead_tok, const int32_t* lead_off,
                                    const int32_t* params, int32_t* state, int64_t* seq, int64_t* segs, int64_t ld_seq, int64_t max_len,
                                    int64_t track_full, int64_t pad, int64_t* tok_out, int64_t* seg_out, int32_t* running, emo_stream_t stream) {
    EMO_CHECK(logits && u_steps && ev_flags && ev_beat && lead_tok && lead_off && params && state && seq && segs && tok_out && seg_out && running,
              "emo_acc_grammar_step: null pointer");
    EMO_CHECK(n > 0 && n_u > 0 && ld_seq > 0 && max_len > 0, "emo_acc_grammar_step: bad sizes");
    EMO_CHECK(V > 0 && V <= 1024, "emo_acc_grammar_step: V must be <= 1024 (got %lld)", (long long)V);
    EMO_CHECK(temperature > 0.f, "emo_acc_grammar_step: temperature must be > 0");
    hipLaunchKernelGGL(acc_grammar_kernel, dim3((unsigned)n), dim3(512), 0, (hipStream_t)stream, logits, n, V, temperature, top_p, u_steps, n_u,
                       ev_flags, ev_beat, lead_tok, lead_off, params, state, seq, segs, ld_seq, max_len, track_full, pad, tok_out, seg_out, running);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

extern "C" int emo_acc_window_step(const float* logits, int64_t m, int64_t V, float temperature, float top_p, const float* u_steps, int64_t n_u,
                                   int64_t ld_u, const int32_t* rows, const int32_t* ev_flags, const int32_t* ev_beat, const int64_t* lead_tok,
                                   const int32_t* lead_off, const int32_t* params, int32_t* state, int64_t* seq, int64_t* segs, int64_t ld_seq,
                                   int64_t window, int64_t track_full, int64_t* win_tok, int64_t* win_seg, int32_t* running, emo_stream_t stream) {
    EMO_CHECK(logits && u_steps && ev_flags && ev_beat && lead_tok && lead_off && params && state && seq && segs && win_tok && win_seg && running,
              "emo_acc_window_step: null pointer");
    EMO_CHECK(m > 0 && n_u > 0 && ld_u > 0 && window > 0 && ld_seq >= window, "emo_acc_window_step: bad sizes");
    EMO_CHECK(V > 0 && V <= 1024, "emo_acc_window_step: V must be <= 1024 (got %lld)", (long long)V);
    EMO_CHECK(temperature > 0.f, "emo_acc_window_step: temperature must be > 0");
    hipLaunchKernelGGL(acc_window_kernel, dim3((unsigned)m), dim3(512), 0, (hipStream_t)stream, logits, V, temperature, top_p, u_steps, n_u, ld_u, rows,
                       ev_flags, ev_beat, lead_tok, lead_off, params, state, seq, segs, ld_seq, window, track_full, win_tok, win_seg, running);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
