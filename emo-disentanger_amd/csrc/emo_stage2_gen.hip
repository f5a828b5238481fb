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
// The ACC_WINDOW kind is the same draw and grammar (acc_draw below, shared) for streams past the window (reference :252-277: the model input is
// the last max_dec_inp_len tokens, positions restarting at 0): nothing is fed token by token; after an acceptance the stream's next model input
// win_tok / win_seg[b, 0..W) = seq / segs[r, LEN - W .. LEN) is written, an injected bar included.
// The ACC_QUEUE kind is the in-window step (acc_stream_step below, shared with ACC) for more jobs than batch rows: a slot b works on job slot_job[b],
// and in the launch in which the job leaves RUNNING thread 0 takes the next open job from queue_head, feeds its first token and flags the row in
// row_reset (emo_hip.h: EMO_GRAMMAR_ACC_QUEUE).  The position of every token fed goes to mem_lens[b], the decode engine's position array.
// All kinds, when the caller wants them (tok_logp / tok_rank / tok_entropy): the figures of the ACCEPTED draw, from the same logits row at
// temperature 1, go to the cell of the token it appended (emo_draw_scores.h) — after the draw loop has ended, since the redraws read the sorted
// state, and by the whole workgroup: whether and where a draw was accepted is read from the LDS state words thread 0 wrote before the loop's
// last barrier.
// All kinds, optional sampling controls (tok_mask / mask_of / temp_of / top_p_of and tok_bias / bias_of / top_k_of / min_p_of, indexed by the
// stream r as params is: emo_grammar_controls): a banned token's logit is read as -inf and a biased one as l + bias by the draw and by nothing
// else, and the draw's candidate count is cut by top_k and min_p behind top-p (the redraws of a launch use the same count): the scores above
// are still the model's, from the row as it wrote it, and primer tokens, injected bars and track_full are fed whether banned or not.
// Kind ACC, optional classifier-free guidance (guide_cond / guide_uncond / guide_scale: emo_hip.h): a guided piece is two rows of the batch, a
// leader on the conditioned primer and a follower on the unconditioned one.  Both workgroups draw from the same combination of the same two
// logits rows with the same uniform and run the same grammar, so the follower stays token for token with its leader and no workgroup reads or
// writes another's state; the scores stay those of each row's own logits.
// Kinds ACC and ACC_QUEUE, optional kept bars (keep_tok / keep_beg / keep_end: emo_hip.h): when the accepted Track_LeadSheet opens a bar the caller
// already has, thread 0 writes the bar out behind the injected lead-sheet bar in the same launch, closes it, and goes on through consecutive kept
// bars (acc_keep_chain below, between the barriers that were there); the feed path then hands the tokens out one per launch.  They are no draws:
// S_ACCEPTED, S_DRAWS and the score cell belong to the Track_LeadSheet alone.  inference._Stream._open_bar is the rule on the host.
#include "emo_grammar.h"

namespace {

// The draws of one launch of one stream, shared by the in-window and the windowed step: draw until the grammar accepts or ends the stream.
// `draws` advances in every thread alike, and thread 0 runs the grammar on the LDS copy of the state (kept there, not in registers, across the
// draws); it alone gets the status back (the other threads: RUNNING).  Besides the block, what differs per call: l the accessor of the stream's
// logits (emo_nucleus.h: its row under its ban, or the guided combination of two rows), u_col its column of the uniform table (pitch a.ld_u),
// row / srow its token and segment rows, ctl its sampling controls (emo_grammar_controls: the ban and the bias are the accessor's and reach
// the first draw's sort, which the redraws reuse with the same two cuts; the scores are taken by the caller from the row as the model wrote it).
// Thread 0, after an accepted Track_LeadSheet has opened bar k (its lead-sheet bar and track_full are at the end of the row, `len` tokens long):
// the chain of consecutive kept bars from k on (emo_hip.h: keep_tok).  WRITE false walks it without touching the row, so the caller tests the
// whole chain against ld_seq before it writes anything; both walks take the same path.  -> RUNNING (bar k, or the bar behind the chain, is
// drawn), DONE (max_events inside a kept bar, or the last bar was kept: closed with keep_eos) or OVERFLOW (the row, a table or a range is too
// short); len / bars as the chain leaves them, kept: whether bar k was kept.  At most TARGET_BARS turns, each bounded by its table range.
template <bool WRITE>
__device__ __forceinline__ int32_t acc_keep_chain(const emo_grammar_step_t& a, const int32_t* spr, int64_t track_ls, int64_t* __restrict__ row,
                                                  int64_t* __restrict__ srow, int32_t k, int32_t& len, int32_t& bars, bool& kept) {
    const int32_t target = spr[EMO_ACC_P_TARGET_BARS], n_bars = spr[EMO_ACC_P_N_BARS], max_events = spr[EMO_ACC_P_MAX_EVENTS];
    const int64_t bar0 = spr[EMO_ACC_P_BAR0], ld_seq = a.ld_seq;
    auto put = [&](int64_t tok, int64_t seg) {
        if (WRITE) {
            row[len] = tok;
            srow[len] = seg;
        }
        ++len;
    };
    while (k >= 0 && k < target && k < n_bars) {
        const int32_t kb = a.keep_beg[bar0 + k], ke = a.keep_end[bar0 + k];
        if (kb < 0) break;                                   // bar k is drawn
        if (ke < kb || ke > a.n_keep) return EMO_ACC_OVERFLOW;
        kept = true;
        for (int32_t i = kb; i < ke; ++i) {
            if (len + 1 > ld_seq) return EMO_ACC_OVERFLOW;
            put(a.keep_tok[i], 1);
            if (len > max_events) return EMO_ACC_DONE;
        }
        if (k == target - 1) {                               // the last bar: closed like a drawn EOS
            if (len + 1 > ld_seq) return EMO_ACC_OVERFLOW;
            put(a.keep_eos, 1);
            return EMO_ACC_DONE;
        }
        if (k + 1 >= n_bars) return EMO_ACC_OVERFLOW;        // closed like a drawn Track_LeadSheet: the next lead-sheet bar, track_full
        const int32_t a0 = a.lead_off[bar0 + k + 1], b = a.lead_off[bar0 + k + 2];
        if (b < a0 || (int64_t)len + 1 + (b - a0) + 1 > ld_seq) return EMO_ACC_OVERFLOW;
        put(track_ls, 0);
        for (int32_t i = a0; i < b; ++i) put(a.lead_tok[i], 0);
        put(a.track_full, 1);
        ++bars;
        ++k;
    }
    return EMO_ACC_RUNNING;
}

// (KEEP: the block has the kept-bar tables; false: the code as it was before they existed.)
template <bool KEEP, typename Logits>
__device__ __forceinline__ int32_t acc_draw(const emo_grammar_step_t& a, const emo_grammar_controls_t ctl, const Logits l, const float* __restrict__ u_col,
                                            int64_t* __restrict__ row, int64_t* __restrict__ srow, const int32_t* spr, int32_t* sst, int32_t* sagain_p,
                                            char* lds, int tid, int32_t& draws) {
    const int64_t V = a.n_token, ld_seq = a.ld_seq;
    int32_t& sagain = *sagain_p;
    int32_t status = EMO_ACC_RUNNING;
    const int32_t draws0 = draws;
    for (;;) {
        if (draws >= a.n_u) {                                // the caller's uniform table is exhausted: never read past it
            status = EMO_ACC_OUT_OF_DRAWS;
            break;
        }
        // a redraw from the same logits needs only the cut and the pick over the sorted state the first draw left in LDS (the same operations
        // on the same data: the id a fresh emo_nucleus_draw with this uniform would give)
        const float u = u_col[(int64_t)draws * a.ld_u];
        const int64_t word = draws == draws0 ? emo_nucleus_draw_from(l, V, ctl.temp, ctl.top_p, ctl.top_k, ctl.min_p, u, lds, tid, [] { __syncthreads(); })
                                            : emo_nucleus_pick(V, ctl.top_p, ctl.top_k, ctl.min_p, u, lds, tid, [] { __syncthreads(); });
        ++draws;
        if (tid == 0) {
            const int32_t fl = a.ev_flags[word], target = spr[EMO_ACC_P_TARGET_BARS], bars = sst[EMO_ACC_S_BARS];
            int32_t len = sst[EMO_ACC_S_LEN];
            bool reject = false;
            if (spr[EMO_ACC_P_SKIP_CHECK] == 0 && (fl & EMO_ACC_EV_BEAT)) {   // Beat positions never go back inside a bar
                const int32_t pos = a.ev_beat[word];
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
                    const int32_t a0 = have ? a.lead_off[j] : 0, b = have ? a.lead_off[j + 1] : 0;
                    bool fits = !((more && (!have || b < a0)) || len + 1 + (more ? b - a0 + 1 : 0) > ld_seq);
                    if constexpr (KEEP) {                    // the kept bars behind the one this opens: walked once, tested before any write
                        if (fits && more) {
                            int32_t len2 = len + 1 + (b - a0) + 1, bars2 = bars + 1;
                            bool kept = false;
                            if (acc_keep_chain<false>(a, spr, word, row, srow, bars + 1, len2, bars2, kept) == EMO_ACC_OVERFLOW) {
                                fits = false;
                                --draws;                     // (thread 0's copy, the one that is stored: the counters as before the draw)
                            }
                        }
                    }
                    if (!fits) {
                        status = EMO_ACC_OVERFLOW;
                    } else {
                        row[len] = word;
                        srow[len++] = 0;
                        sst[EMO_ACC_S_BARS] = bars + 1;
                        ++sst[EMO_ACC_S_ACCEPTED];
                        if (more) {
                            for (int32_t i = a0; i < b; ++i) {
                                row[len] = a.lead_tok[i];
                                srow[len++] = 0;
                            }
                            row[len] = a.track_full;
                            srow[len++] = 1;
                            sst[EMO_ACC_S_CUR_POS] = 0;
                            if constexpr (KEEP) {
                                int32_t bars2 = bars + 1;
                                bool kept = false;
                                status = acc_keep_chain<true>(a, spr, word, row, srow, bars + 1, len, bars2, kept);
                                sst[EMO_ACC_S_BARS] = bars2;
                                if (kept) sst[EMO_ACC_S_FAILED] = 0;
                            }
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

// One token step of stream r (kind ACC: a stream of the batch; kind ACC_QUEUE: a job) in batch row b, whose logits row it draws from and whose
// next input it writes, after emo_grammar_open has brought the stream's words to sst / spr and found it RUNNING.  All 512 threads call it; every
// barrier inside lies on a path that sst, spr and the launch arguments alone decide.  Thread 0 leaves the stream's state words in memory.
// CTL: the block has sampling controls (emo_grammar_controls).  GUIDE (kind ACC alone): the block has the three guidance tables; a stream whose
// pair (guide_cond[r], guide_uncond[r]) is two distinct rows of the batch draws from their combination (emo_guided_logits) with the uniforms of
// column guide_cond[r], every other stream as without them.  The pair is the same word in every thread, so the barriers stay uniform.  The
// scores are still taken from the stream's own row b.
template <bool CTL, bool GUIDE, bool KEEP>
__device__ __forceinline__ void acc_stream_step(const emo_grammar_step_t& a, int64_t b, int64_t r, char* lds, int32_t* sst, const int32_t* spr,
                                                int32_t* sagain, float* sred, int tid) {
    int32_t* st = a.state + r * EMO_ACC_STATE_WORDS;
    int64_t* row = a.seq + r * a.ld_seq;
    int64_t* srow = a.segs + r * a.ld_seq;
    if (sst[EMO_ACC_S_LEN] >= a.max_len) {                   // checked before the feed test, like the host loop's `overflow`
        if (tid == 0) {
            st[EMO_ACC_S_STATUS] = EMO_ACC_WINDOW;
            atomicSub(a.running, 1);
            a.tok_out[b] = a.pad;
            a.seg_out[b] = 1;
        }
        return;
    }
    int32_t consumed = sst[EMO_ACC_S_CONSUMED];
    if (consumed < sst[EMO_ACC_S_LEN]) {
        if (tid == 0) {
            a.tok_out[b] = row[consumed];
            a.seg_out[b] = srow[consumed];
            st[EMO_ACC_S_CONSUMED] = consumed + 1;
        }
        return;
    }
    int32_t draws = sst[EMO_ACC_S_DRAWS];
    // (read before thread 0 can have touched the state: it writes only behind the barriers of the first draw)
    const bool scores = emo_grammar_wants_scores(a);
    const int32_t len0 = scores ? sst[EMO_ACC_S_LEN] : 0, acc0 = scores ? sst[EMO_ACC_S_ACCEPTED] : 0;
    const emo_grammar_controls_t ctl = emo_grammar_controls<CTL>(a, r);
    int32_t status;
    int64_t gc = -1, gu = -1;
    if constexpr (GUIDE) {
        gc = a.guide_cond[r];
        gu = a.guide_uncond[r];
    }
    if (GUIDE && gc != gu && gc >= 0 && gc < a.n_rows && gu >= 0 && gu < a.n_rows)      // (both rows of a pair add the LEADER's bias row)
        status = acc_draw<KEEP>(a, ctl, emo_guided_logits{a.logits + gc * a.n_token, a.logits + gu * a.n_token, a.guide_scale[r], ctl.ban,
                                                          emo_grammar_controls<CTL>(a, gc).bias}, a.u_steps + gc, row, srow, spr, sst, sagain, lds, tid, draws);
    else
        status = acc_draw<KEEP>(a, ctl, emo_banned_logits{a.logits + b * a.n_token, ctl.ban, ctl.bias}, a.u_steps + r, row, srow, spr, sst, sagain, lds, tid, draws);
    // an acceptance appended its word at the old length (an injected bar follows it) and counted itself, in front of the loop's last barrier
    if (scores && sst[EMO_ACC_S_ACCEPTED] != acc0) emo_grammar_score(a, a.logits + b * a.n_token, r, len0, row[len0], sred, tid);
    if (tid != 0) return;
    if (status == EMO_ACC_RUNNING) {                         // the accepted word (or Track_LeadSheet before an injected bar) is the next input
        a.tok_out[b] = row[consumed];
        a.seg_out[b] = srow[consumed];
        ++consumed;
    } else {
        a.tok_out[b] = a.pad;
        a.seg_out[b] = 1;
        atomicSub(a.running, 1);
    }
    sst[EMO_ACC_S_STATUS] = status;
    sst[EMO_ACC_S_CONSUMED] = consumed;
    sst[EMO_ACC_S_DRAWS] = draws;
    for (int i = 0; i < EMO_ACC_STATE_WORDS; ++i) st[i] = sst[i];
}

template <bool CTL, bool GUIDE, bool KEEP>
__global__ __launch_bounds__(512) void acc_grammar_kernel(const emo_grammar_step_t a) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_ACC_STATE_WORDS], spr[EMO_ACC_PARAM_WORDS], sagain;
    __shared__ float sred[EMO_DRAW_SCORES_WORDS];
    const int tid = (int)threadIdx.x;
    const int64_t r = blockIdx.x;
    emo_grammar_open(a.state + r * EMO_ACC_STATE_WORDS, EMO_ACC_STATE_WORDS, a.params + r * EMO_ACC_PARAM_WORDS, EMO_ACC_PARAM_WORDS, sst, spr, tid);
    if (sst[EMO_ACC_S_STATUS] != EMO_ACC_RUNNING) {
        if (tid == 0) {
            a.tok_out[r] = a.pad;
            a.seg_out[r] = 1;
        }
        return;
    }
    acc_stream_step<CTL, GUIDE, KEEP>(a, r, r, lds, sst, spr, &sagain, sred, tid);
}

// Thread 0 of slot b, whose job (if it had one) is over: the next queued job that is RUNNING, or none.  queue_head only grows, so a slot that
// has seen it at n_jobs never adds to it again.
__device__ __forceinline__ void acc_queue_admit(const emo_grammar_step_t& a, int64_t b) {
    int32_t next = -1;
    while (__atomic_load_n(a.queue_head, __ATOMIC_RELAXED) < a.n_jobs) {
        const int32_t h = atomicAdd(a.queue_head, 1);
        if (h >= a.n_jobs) break;
        if (a.state[(int64_t)h * EMO_ACC_STATE_WORDS + EMO_ACC_S_STATUS] == EMO_ACC_RUNNING) {      // (a job closed on the host is passed over)
            next = h;
            break;
        }
    }
    a.slot_job[b] = next;
    a.mem_lens[b] = 0;                                       // the row of the model starts again at position 0; a free slot stays there
    a.row_reset[b] = next >= 0 ? 1 : 0;
    if (next >= 0) {
        a.tok_out[b] = a.seq[(int64_t)next * a.ld_seq];      // the model step behind this launch is the new job's first token
        a.seg_out[b] = a.segs[(int64_t)next * a.ld_seq];
        a.state[(int64_t)next * EMO_ACC_STATE_WORDS + EMO_ACC_S_CONSUMED] = 1;
    } else {
        a.tok_out[b] = a.pad;
        a.seg_out[b] = 1;
    }
}

template <bool CTL, bool KEEP>
__global__ __launch_bounds__(512) void acc_queue_kernel(const emo_grammar_step_t a) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_ACC_STATE_WORDS], spr[EMO_ACC_PARAM_WORDS], sagain, sslot;
    __shared__ float sred[EMO_DRAW_SCORES_WORDS];
    const int tid = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid == 0) sslot = a.slot_job[b];                     // thread 0 writes slot_job[b] below: the others decide from this copy
    __syncthreads();
    const int64_t j = sslot;
    if (j < 0 || j >= a.n_jobs) {                            // a free slot
        if (tid == 0) acc_queue_admit(a, b);
        return;
    }
    int32_t* st = a.state + j * EMO_ACC_STATE_WORDS;
    emo_grammar_open(st, EMO_ACC_STATE_WORDS, a.params + j * EMO_ACC_PARAM_WORDS, EMO_ACC_PARAM_WORDS, sst, spr, tid);
    if (sst[EMO_ACC_S_STATUS] == EMO_ACC_RUNNING) {
        if (sst[EMO_ACC_S_LEN] < a.max_len && sst[EMO_ACC_S_CONSUMED] >= a.mem_rows) {      // the token of this step has no position: never fed
            if (tid == 0) {
                st[EMO_ACC_S_STATUS] = EMO_ACC_OVERFLOW;
                atomicSub(a.running, 1);
            }
        } else {
            acc_stream_step<CTL, false, KEEP>(a, b, j, lds, sst, spr, &sagain, sred, tid);
        }
    }
    if (tid != 0) return;
    if (st[EMO_ACC_S_STATUS] == EMO_ACC_RUNNING) {           // (thread 0 reads what it wrote itself)
        a.mem_lens[b] = st[EMO_ACC_S_CONSUMED] - 1;          // the position of the token this launch feeds: its index in seq[j]
        a.row_reset[b] = 0;
    } else {
        if (a.job_steps) a.job_steps[j] = st[EMO_ACC_S_CONSUMED];    // tokens the model was fed for the job = launches it held the slot
        acc_queue_admit(a, b);
    }
}

template <bool CTL>
__global__ __launch_bounds__(512) void acc_window_kernel(const emo_grammar_step_t a) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_ACC_STATE_WORDS], spr[EMO_ACC_PARAM_WORDS], sagain;
    __shared__ float sred[EMO_DRAW_SCORES_WORDS];
    const int tid = (int)threadIdx.x;
    const int64_t b = blockIdx.x;                            // row of the batch: logits, win_tok, win_seg
    const int64_t r = a.rows ? a.rows[b] : b;                // the stream: state, params, seq, segs, column of u_steps
    if (r < 0 || r >= a.ld_u) return;                        // (not a stream of the table: nothing is read or written for it)
    const int64_t W = a.window;
    int32_t* st = a.state + r * EMO_ACC_STATE_WORDS;
    int64_t* row = a.seq + r * a.ld_seq;
    int64_t* srow = a.segs + r * a.ld_seq;
    emo_grammar_open(st, EMO_ACC_STATE_WORDS, a.params + r * EMO_ACC_PARAM_WORDS, EMO_ACC_PARAM_WORDS, sst, spr, tid);
    if (sst[EMO_ACC_S_STATUS] != EMO_ACC_RUNNING) return;    // finished: its window row stays as it is
    if (sst[EMO_ACC_S_LEN] < W || sst[EMO_ACC_S_LEN] > a.ld_seq) {  // no full window to read: a caller error, never a read outside the row
        if (tid == 0) {
            st[EMO_ACC_S_STATUS] = EMO_ACC_OVERFLOW;
            atomicSub(a.running, 1);
        }
        return;
    }
    int32_t draws = sst[EMO_ACC_S_DRAWS];
    const bool scores = emo_grammar_wants_scores(a);         // as in acc_grammar_kernel; the tables are indexed by the stream r, the logits by b
    const int32_t len0 = scores ? sst[EMO_ACC_S_LEN] : 0, acc0 = scores ? sst[EMO_ACC_S_ACCEPTED] : 0;
    const emo_grammar_controls_t ctl = emo_grammar_controls<CTL>(a, r);
    const int32_t status = acc_draw<false>(a, ctl, emo_banned_logits{a.logits + b * a.n_token, ctl.ban, ctl.bias}, a.u_steps + r, row, srow, spr, sst, &sagain, lds, tid, draws);
    if (scores && sst[EMO_ACC_S_ACCEPTED] != acc0) emo_grammar_score(a, a.logits + b * a.n_token, r, len0, row[len0], sred, tid);
    if (tid == 0) {
        if (status != EMO_ACC_RUNNING) atomicSub(a.running, 1);
        sst[EMO_ACC_S_STATUS] = status;
        sst[EMO_ACC_S_DRAWS] = draws;
        for (int i = 0; i < EMO_ACC_STATE_WORDS; ++i) st[i] = sst[i];
    }
    __syncthreads();                                         // thread 0's status, length and new tokens are visible to the workgroup
    if (sst[EMO_ACC_S_STATUS] != EMO_ACC_RUNNING) return;
    const int64_t off = (int64_t)sst[EMO_ACC_S_LEN] - W;     // >= 0: the length only grows
    for (int64_t i = tid; i < W; i += 512) {
        a.win_tok[b * W + i] = row[off + i];
        a.win_seg[b * W + i] = srow[off + i];
    }
}

}  // namespace

extern "C" int emo_grammar_step_size(void) { return (int)sizeof(emo_grammar_step_t); }

extern "C" int emo_grammar_step(const emo_grammar_step_t* args, emo_stream_t stream) {
    EMO_CHECK(args, "emo_grammar_step: null argument block");
    const emo_grammar_step_t& a = *args;
    EMO_CHECK(a.kind >= 0 && a.kind <= 4, "emo_grammar_step: kind %d is none of 0 (TXL), 1 (ACC), 2 (ACC_WINDOW), 3 (TXL_QUEUE), 4 (ACC_QUEUE)", (int)a.kind);
    const bool tq = a.kind == EMO_GRAMMAR_TXL_QUEUE, aq = a.kind == EMO_GRAMMAR_ACC_QUEUE, queue = tq || aq;
    const bool txl = a.kind == EMO_GRAMMAR_TXL || tq, acc = a.kind == EMO_GRAMMAR_ACC || aq;
    const char* const name = tq ? "txl_queue" : aq ? "acc_queue" : txl ? "txl" : acc ? "acc" : "acc_window";
    const bool common = a.logits && a.u_steps && a.ev_flags && a.ev_beat && a.params && a.state && a.seq && a.running;
    const bool lead = a.lead_tok && a.lead_off && a.segs;
    const bool slots = a.slot_job && a.queue_head && a.mem_lens;
    EMO_CHECK(common && (txl ? a.tok_out != nullptr : acc ? lead && a.tok_out && a.seg_out : lead && a.win_tok && a.win_seg) && (!queue || slots) &&
                  (!aq || a.row_reset),
              "emo_grammar_step[%s]: null pointer", name);
    // (TXL, ACC: workgroup r reads column r of the uniform table; the queue kinds: job j reads column j)
    EMO_CHECK(a.n_rows > 0 && a.n_u > 0 && a.ld_u > 0 && a.ld_seq > 0 &&
                  (queue ? a.n_jobs > 0 && a.ld_u >= a.n_jobs && a.mem_rows > 0 && a.n_jobs <= INT32_MAX - a.n_rows : txl || acc ? a.ld_u >= a.n_rows : a.window > 0 && a.ld_seq >= a.window) &&
                  (!acc || a.max_len > 0),
              "emo_grammar_step[%s]: bad sizes", name);
    EMO_CHECK(a.n_token > 0 && a.n_token <= 1024, "emo_grammar_step[%s]: V must be <= 1024 (got %lld)", name, (long long)a.n_token);
    if (txl) {
        EMO_CHECK(a.temperature > 0.f && a.key_temperature > 0.f, "emo_grammar_step[%s]: temperatures must be > 0", name);
        // (kind TXL reads the guidance tables as kind ACC does, TXL_QUEUE ignores them: the check comes behind every other one of the kind)
        const int txl_guide = tq ? 0 : (a.guide_cond != nullptr) + (a.guide_uncond != nullptr) + (a.guide_scale != nullptr);
        EMO_CHECK(txl_guide == 0 || txl_guide == 3, "emo_grammar_step[%s]: guide_cond, guide_uncond and guide_scale come together or not at all", name);
        // (both kinds read the kept-bar tables and keep_left; a block without them launches a <.., false> instance, the kernel as it was before they existed)
        const int txl_keep = (a.keep_tok != nullptr) + (a.keep_beg != nullptr) + (a.keep_end != nullptr) + (a.keep_left != nullptr);
        EMO_CHECK(txl_keep == 0 || (txl_keep == 4 && a.n_keep >= 0 && a.n_keep <= INT32_MAX),
                  "emo_grammar_step[%s]: keep_tok, keep_beg, keep_end and keep_left come together or not at all, with 0 <= n_keep < 2^31", name);
        EMO_CHECK(txl_keep == 0 || (a.keep_bar >= 0 && a.keep_bar < a.n_token), "emo_grammar_step[%s]: keep_bar %lld lies outside [0, V)", name,
                  (long long)a.keep_bar);
        // (the bias table comes with the map that reads it and with its row count; asked last, behind every other refusal of the kind)
        EMO_CHECK(!a.tok_bias || (a.bias_of && a.n_biases > 0), "emo_grammar_step[%s]: tok_bias needs bias_of and n_biases > 0 (got n_biases %lld)", name,
                  (long long)a.n_biases);
        return tq ? emo_txl_queue_launch(a, stream) : emo_txl_grammar_launch(a, stream);
    }
    EMO_CHECK(a.temperature > 0.f, "emo_grammar_step[%s]: temperature must be > 0", name);
    // (the <false> instances are the kernels as they were before the sampling controls: a block without any launches those)
    const bool ctl = emo_grammar_has_controls(a);
    // (of the kinds below ACC alone reads the guidance tables; a block without them launches the <.., false> instance, the kernel as it was before they existed)
    const int guide = a.kind == EMO_GRAMMAR_ACC ? (a.guide_cond != nullptr) + (a.guide_uncond != nullptr) + (a.guide_scale != nullptr) : 0;
    EMO_CHECK(guide == 0 || guide == 3, "emo_grammar_step[%s]: guide_cond, guide_uncond and guide_scale come together or not at all", name);
    // (kinds ACC and ACC_QUEUE read the kept-bar tables; a block without them launches a <.., false> instance, the kernel as it was before they
    // existed: six instances are new, the four of ACC and the two of ACC_QUEUE; ACC_WINDOW has none and ignores the tables)
    const int keep = acc ? (a.keep_tok != nullptr) + (a.keep_beg != nullptr) + (a.keep_end != nullptr) : 0;
    EMO_CHECK(keep == 0 || (keep == 3 && a.n_keep >= 0 && a.n_keep <= INT32_MAX),
              "emo_grammar_step[%s]: keep_tok, keep_beg and keep_end come together or not at all, with 0 <= n_keep < 2^31", name);
    // (the bias table comes with the map that reads it and with its row count; asked last, behind every other refusal of the kind)
    EMO_CHECK(!a.tok_bias || (a.bias_of && a.n_biases > 0), "emo_grammar_step[%s]: tok_bias needs bias_of and n_biases > 0 (got n_biases %lld)", name,
              (long long)a.n_biases);
    const auto kernel = aq       ? (keep ? (ctl ? acc_queue_kernel<true, true> : acc_queue_kernel<false, true>)
                                         : (ctl ? acc_queue_kernel<true, false> : acc_queue_kernel<false, false>))
                        : !acc   ? (ctl ? acc_window_kernel<true> : acc_window_kernel<false>)
                        : keep   ? (guide ? (ctl ? acc_grammar_kernel<true, true, true> : acc_grammar_kernel<false, true, true>)
                                          : (ctl ? acc_grammar_kernel<true, false, true> : acc_grammar_kernel<false, false, true>))
                        : guide  ? (ctl ? acc_grammar_kernel<true, true, false> : acc_grammar_kernel<false, true, false>)
                                 : (ctl ? acc_grammar_kernel<true, false, false> : acc_grammar_kernel<false, false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.n_rows), dim3(512), 0, (hipStream_t)stream, a);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

// ---------------------------------------------------------------------------------------------- re-anchoring on a bar (emo_acc_rebase)
// A stream that filled the window (status WINDOW) drops its oldest whole bars and keeps its primer: the context the model was trained on (the
// reference dataloader, dataloader.py:179-186: the piece's opening events followed by the piece from a random bar on, positions from 0).  One
// 512-thread workgroup per row.  The cut b is found by a strided scan of the row (every thread keeps the smallest bar start at or behind the
// first index that fits `keep`, and the largest bar start of all), a wave reduction (wave size 64) and a reduction across the 8 waves through
// LDS; inference.rebase_plan is the rule on the host.  The row is then copied, primer + tail, into the destination row (another buffer: source
// and destination never alias), the dropped tokens and their recorded scores go to the row's archive, and thread 0 writes the state and
// parameter words of the new phase.  Every global read of a word that thread 0 rewrites lies in front of the first barrier.
namespace {

__global__ __launch_bounds__(512) void acc_rebase_kernel(const emo_acc_rebase_t a) {
    __shared__ int32_t smin[8], smax[8], scur;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    int32_t* st = a.state + r * EMO_ACC_STATE_WORDS;
    if (st[EMO_ACC_S_STATUS] != EMO_ACC_WINDOW) {            // (nobody writes the word in this branch: every thread reads the same value)
        if (tid == 0) a.new_len[r] = 0;
        return;
    }
    const int64_t n = st[EMO_ACC_S_LEN], P = a.primer_len[r];
    const int64_t* row = a.seq + r * a.ld_seq;
    const int64_t* srow = a.segs + r * a.ld_seq;
    if (tid == 0) scur = a.arch_len[r];
    const bool sane = P >= 0 && P <= n && n <= a.ld_seq;     // a row that cannot be read is a caller error (OVERFLOW below), never a read outside it
    const int64_t first = P + n - a.keep > P ? P + n - a.keep : P;      // bar starts at or behind it leave at most `keep` tokens
    int32_t lo = INT32_MAX, hi = -1;
    if (sane) {
        for (int64_t i = P + tid; i < n; i += 512) {
            if (row[i] == a.track_leadsheet) {
                if (i >= first && (int32_t)i < lo) lo = (int32_t)i;
                hi = (int32_t)i;                             // (i grows: the last one seen is the thread's largest)
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) {
        smin[wave] = lo;
        smax[wave] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        lo = smin[w] < lo ? smin[w] : lo;
        hi = smax[w] > hi ? smax[w] : hi;
    }
    int64_t b = P;
    int32_t err = 0;
    if (!sane) err = EMO_ACC_OVERFLOW;
    else if (lo != INT32_MAX) b = lo;
    else if (hi >= 0 && P + n - hi <= a.window - a.longest_bar - 2) b = hi;
    else err = EMO_REBASE_BAR_TOO_LONG;
    const int64_t drop = b - P, len2 = P + n - b, cur = scur;
    if (!err && (len2 > a.ld_dst || cur < 0 || cur + drop > a.ld_arch)) err = EMO_ACC_OVERFLOW;
    if (err) {
        if (tid == 0) {
            st[EMO_ACC_S_STATUS] = err;
            a.new_len[r] = 0;
        }
        return;
    }
    const bool scores = a.tok_logp != nullptr;                   // (the entry takes the three sources and destinations together or not at all)
    const float nan = __builtin_nanf("");
    for (int64_t i = tid; i < a.ld_dst; i += 512) {
        const int64_t s = i < P ? i : b + (i - P);
        const bool in = i < len2;
        a.dst_seq[r * a.ld_dst + i] = in ? row[s] : a.pad;
        a.dst_segs[r * a.ld_dst + i] = in ? srow[s] : 1;
        if (scores) {
            a.dst_logp[r * a.ld_dst + i] = in ? a.tok_logp[r * a.ld_seq + s] : nan;
            a.dst_rank[r * a.ld_dst + i] = in ? a.tok_rank[r * a.ld_seq + s] : -1;
            a.dst_entropy[r * a.ld_dst + i] = in ? a.tok_entropy[r * a.ld_seq + s] : nan;
        }
    }
    for (int64_t j = tid; j < drop; j += 512) {
        a.arch_tok[r * a.ld_arch + cur + j] = row[P + j];
        if (scores) {
            a.arch_logp[r * a.ld_arch + cur + j] = a.tok_logp[r * a.ld_seq + P + j];
            a.arch_rank[r * a.ld_arch + cur + j] = a.tok_rank[r * a.ld_seq + P + j];
            a.arch_entropy[r * a.ld_arch + cur + j] = a.tok_entropy[r * a.ld_seq + P + j];
        }
    }
    if (tid != 0) return;
    a.arch_len[r] = (int32_t)(cur + drop);
    st[EMO_ACC_S_STATUS] = EMO_ACC_RUNNING;
    st[EMO_ACC_S_LEN] = (int32_t)len2;
    st[EMO_ACC_S_CONSUMED] = (int32_t)len2;                  // the prefill of the phase takes the whole context
    st[EMO_ACC_S_DRAWS] = 0;
    a.params[r * EMO_ACC_PARAM_WORDS + EMO_ACC_P_MAX_EVENTS] -= (int32_t)drop;     // the whole-piece limit, in the new row's indices
    a.new_len[r] = (int32_t)len2;
    atomicAdd(a.running, 1);
}

}  // namespace

extern "C" int emo_acc_rebase_size(void) { return (int)sizeof(emo_acc_rebase_t); }

extern "C" int emo_acc_rebase(const emo_acc_rebase_t* args, emo_stream_t stream) {
    EMO_CHECK(args, "emo_acc_rebase: null argument block");
    const emo_acc_rebase_t& a = *args;
    EMO_CHECK(a.seq && a.segs && a.state && a.params && a.primer_len && a.dst_seq && a.dst_segs && a.arch_tok && a.arch_len && a.new_len && a.running,
              "emo_acc_rebase: null pointer");
    EMO_CHECK(a.n_rows > 0 && a.ld_seq > 0 && a.ld_dst > 0 && a.ld_arch > 0 && a.ld_seq <= INT32_MAX && a.ld_dst <= INT32_MAX && a.ld_arch <= INT32_MAX,
              "emo_acc_rebase: bad sizes");
    EMO_CHECK(a.longest_bar >= 0 && a.keep > 0 && a.keep <= a.window - a.longest_bar - 2 && a.window <= a.ld_dst,
              "emo_acc_rebase: needs 0 < keep <= window - longest_bar - 2 and rows of at least window tokens (keep %lld, window %lld, longest_bar %lld, ld_dst %lld)",
              (long long)a.keep, (long long)a.window, (long long)a.longest_bar, (long long)a.ld_dst);
    EMO_CHECK(a.dst_seq != a.seq && a.dst_segs != a.segs, "emo_acc_rebase: source and destination rows must not alias");
    const int have = (a.tok_logp != nullptr) + (a.tok_rank != nullptr) + (a.tok_entropy != nullptr) + (a.dst_logp != nullptr) + (a.dst_rank != nullptr) +
                     (a.dst_entropy != nullptr) + (a.arch_logp != nullptr) + (a.arch_rank != nullptr) + (a.arch_entropy != nullptr);
    EMO_CHECK(have == 0 || (have == 9 && a.dst_logp != a.tok_logp && a.dst_rank != a.tok_rank && a.dst_entropy != a.tok_entropy),
              "emo_acc_rebase: the score tables come as three sources, three destinations and three archives that do not alias, or not at all");
    hipLaunchKernelGGL(acc_rebase_kernel, dim3((unsigned)a.n_rows), dim3(512), 0, (hipStream_t)stream, a);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
