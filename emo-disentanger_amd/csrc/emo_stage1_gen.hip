// Stage-1 lead-sheet generation (emo_grammar_step, kind TXL): the sample-and-grammar half of one lock-step token step (reference stage1_compose/inference_utils.py:51-134,
// match_emotion_key :137-142).  One 512-thread workgroup per stream; all loop state lives in device memory (no allocation, graph-capturable).
// The draw is emo_nucleus_draw, the device code of emo_sample_nucleus, so a stream picks the same id from the same logits and uniform.
// Per stream r:
//   finished            -> nothing;
//   feeding the primer  -> a.tok_out[r] = seq[r, feed], feed += 1, no draw (a primer longer than the common prefix, or a re-fed primer);
//   otherwise           -> draw with u_steps[draws, r], run the grammar in the reference's order (key rule, Beat, Bar, PAD, append, end tests)
//                          and choose the next input: the accepted word, the previous input again after a rejection, or — when nothing has
//                          been accepted yet — the whole primer again from its first token (the reference re-submits `generated`).
// When the caller wants them (tok_logp / tok_rank / tok_entropy), an accepted draw's figures go to the cell of the token it appended: from the
// same logits row at temperature 1 — the key draw too, which draws at key_temperature — by the whole workgroup (emo_draw_scores.h), so thread 0
// publishes the accepted column and word through LDS.  A rejection records nothing.
// The optional sampling controls (tok_mask / mask_of / temp_of / top_p_of and tok_bias / bias_of / top_k_of / min_p_of, indexed by the stream r
// as params is: emo_grammar_controls) reach the draw alone: a banned token's logit is read as -inf there and a biased one as l + bias, the
// candidate count is cut by top_k and min_p behind top-p, the scores above are still taken from the row as the model wrote it, and primer
// tokens are fed whether banned or not.  The key draw keeps key_temperature / key_top_p and runs under the ban, the bias and both cuts.
// Kind TXL, optional classifier-free guidance (guide_cond / guide_uncond / guide_scale: emo_hip.h): a guided piece is two rows of the batch, a
// leader on the conditioned primer and a follower on the same primer with the unconditioned token in the emotion's place.  Both workgroups draw
// (the key draw included) from the same combination of the same two logits rows with the leader's uniform and the leader's controls, then each
// runs the grammar on its own row and state: the follower stays token for token with its leader, a rejection or a primer re-feed included, and
// no workgroup reads what another writes in the launch; the scores stay those of each row's own logits.
// Both kinds, optional kept bars (keep_tok / keep_beg / keep_end / keep_left: emo_hip.h): when the accepted Bar opens a bar the caller already has,
// thread 0 writes the bar's content and the Bar that closes it behind the drawn one in the same launch and goes on through consecutive kept bars
// (txl_keep_chain below, between the barriers that were there); keep_left[r] counts what is written and not yet fed, and the launches behind
// hand those tokens out one each without drawing.  They are no draws: S_ACCEPTED, S_DRAWS and the score cell belong to the drawn Bar alone.
// stage1_inference._LeadSheet._open_bar is the rule on the host.
#include "emo_grammar.h"

namespace {

// Thread 0, after an accepted Bar has opened bar `bars` - 1 (the Bar is the row's last token, `len` tokens long): the chain of consecutive kept
// bars from that bar on (emo_hip.h: keep_bar).  WRITE false walks it without touching the row, so the caller tests the whole chain against ld_seq
// before it writes anything; both walks take the same path.  -> RUNNING (the bar, or the bar behind the chain, is drawn), DONE (max_events
// inside a kept bar, or max_bars at a forced Bar) or OVERFLOW (the row or a range is too short); len / bars as the chain leaves them.  At
// most params[KEEP_BARS] turns, each bounded by its table range.
template <bool WRITE>
__device__ __forceinline__ int32_t txl_keep_chain(const emo_grammar_step_t& a, const int32_t* spr, int64_t* __restrict__ row, int32_t& len, int32_t& bars) {
    const int32_t max_bars = spr[EMO_TXL_P_MAX_BARS], max_events = spr[EMO_TXL_P_MAX_EVENTS], n_bars = spr[EMO_TXL_P_KEEP_BARS];
    const int64_t bar0 = spr[EMO_TXL_P_KEEP0], ld_seq = a.ld_seq;
    if (bar0 < 0) return EMO_TXL_RUNNING;
    for (int32_t k = bars - 1; k >= 0 && k < n_bars; ++k) {
        const int32_t kb = a.keep_beg[bar0 + k], ke = a.keep_end[bar0 + k];
        if (kb < 0) break;                                   // bar k is drawn
        if (ke < kb || ke > a.n_keep) return EMO_TXL_OVERFLOW;
        for (int32_t i = kb; i < ke; ++i) {
            if (len + 1 > ld_seq) return EMO_TXL_OVERFLOW;
            if (WRITE) row[len] = a.keep_tok[i];
            if (++len > max_events) return EMO_TXL_DONE;
        }
        if (len + 1 > ld_seq) return EMO_TXL_OVERFLOW;
        if (WRITE) row[len] = a.keep_bar;                    // closes bar k and opens bar k + 1
        ++len;
        ++bars;
        if (len > max_events || bars >= max_bars) return EMO_TXL_DONE;
    }
    return EMO_TXL_RUNNING;
}

// Thread 0's part of a drawing step: the grammar on `word`, the next input (to tok_out[b]), the state.  -> the column of seq[r] the word was
// appended at, or -1.  (KEEP: the block has the kept-bar tables, stream r's count of unfed kept tokens is keep_left[r]; false: the code as it
// was before they existed.)
template <bool KEEP>
__device__ __forceinline__ int32_t txl_grammar(const emo_grammar_step_t& a, int64_t b, int64_t r, int64_t* row, int32_t* st,
                                               const int32_t* sst, const int32_t* spr, int64_t word, int32_t draws, bool key_step, int32_t len) {
    const int32_t len0 = len;
    int32_t kept = 0;                                        // tokens a chain wrote behind the accepted Bar, still to be fed
    bool counted = true;
    const int32_t fl = a.ev_flags[word];
    int32_t status = EMO_TXL_RUNNING, accepted = sst[EMO_TXL_S_ACCEPTED], beat = sst[EMO_TXL_S_BEAT], bars = sst[EMO_TXL_S_BARS];
    int32_t failed = sst[EMO_TXL_S_FAILED], feed = sst[EMO_TXL_S_FEED];
    bool reject = false;
    if (key_step && spr[EMO_TXL_P_KEY_RULE]) {
        if (!(fl & EMO_TXL_EV_KEY)) {
            status = EMO_TXL_KEY_ERROR;                      // reference: ValueError('[info] key generation failed')
        } else {
            const int32_t mode = spr[EMO_TXL_P_EMO_MODE];
            reject = !((mode == 1 && (fl & EMO_TXL_EV_MAJOR)) || (mode == 2 && (fl & EMO_TXL_EV_MINOR)));   // `continue`: no further grammar
        }
    }
    if (status == EMO_TXL_RUNNING && !reject) {
        if (fl & EMO_TXL_EV_BEAT) {                          // Beat positions never decrease inside a bar; 256 rejections in a row abort
            const int32_t pos = a.ev_beat[word];
            if (pos < beat) {
                reject = true;
                if (++failed >= 256) status = EMO_TXL_STUCK;
            } else {
                beat = pos;
                failed = 0;
            }
        }
        if (!reject) {
            if (fl & EMO_TXL_EV_BAR) {
                ++bars;
                beat = 0;
            }
            if (fl & EMO_TXL_EV_PAD) {
                reject = true;                               // not counted toward failed_cnt
            } else if (len >= a.ld_seq) {
                status = EMO_TXL_OVERFLOW;
            } else {
                bool fits = true;
                if constexpr (KEEP) {                        // the kept bars behind a Bar that leaves the stream open: walked once, tested before any write
                    if ((fl & EMO_TXL_EV_BAR) && !(fl & EMO_TXL_EV_EOS) && len + 1 <= spr[EMO_TXL_P_MAX_EVENTS] && bars < spr[EMO_TXL_P_MAX_BARS]) {
                        int32_t len2 = len + 1, bars2 = bars;
                        fits = txl_keep_chain<false>(a, spr, row, len2, bars2) != EMO_TXL_OVERFLOW;
                    }
                }
                if (!fits) {                                 // the row and the counters as before the draw, which is not counted
                    status = EMO_TXL_OVERFLOW;
                    beat = sst[EMO_TXL_S_BEAT];
                    bars = sst[EMO_TXL_S_BARS];
                    failed = sst[EMO_TXL_S_FAILED];
                    counted = false;
                } else {
                    row[len++] = word;
                    ++accepted;
                    if (len > spr[EMO_TXL_P_MAX_EVENTS] || (fl & EMO_TXL_EV_EOS)) status = EMO_TXL_DONE;
                    if constexpr (KEEP) {
                        if (status == EMO_TXL_RUNNING && (fl & EMO_TXL_EV_BAR) && bars < spr[EMO_TXL_P_MAX_BARS]) {
                            const int32_t len1 = len;
                            status = txl_keep_chain<true>(a, spr, row, len, bars);
                            if (len > len1) {                // a kept bar lay behind the Bar: the next drawn bar starts clean
                                beat = 0;
                                failed = 0;
                                if (status == EMO_TXL_RUNNING) kept = len - len1;
                            }
                        }
                    }
                }
            }
        }
    }
    if (status == EMO_TXL_RUNNING && bars >= spr[EMO_TXL_P_MAX_BARS]) status = EMO_TXL_DONE;
    if (status == EMO_TXL_RUNNING && accepted == 0) {
        a.tok_out[b] = row[0];                               // nothing accepted yet: the whole primer again, one token per step
        feed = 1;
    } else {
        a.tok_out[b] = row[len - 1 - kept];                  // the accepted word (a kept chain lies behind it), or after a rejection the previous
    }                                                        // input again (a finished stream's row idles on its last token)
    if constexpr (KEEP) {
        if (kept > 0) a.keep_left[r] = kept;
    }
    st[EMO_TXL_S_STATUS] = status;
    st[EMO_TXL_S_LEN] = len;
    st[EMO_TXL_S_ACCEPTED] = accepted;
    st[EMO_TXL_S_BEAT] = beat;
    st[EMO_TXL_S_BARS] = bars;
    st[EMO_TXL_S_FAILED] = failed;
    st[EMO_TXL_S_FEED] = feed;
    st[EMO_TXL_S_DRAWS] = draws + (counted ? 1 : 0);
    if (status != EMO_TXL_RUNNING) atomicSub(a.running, 1);
    return len > len0 ? len0 : -1;
}

// One token step of stream r (kind TXL: a stream of the batch; kind TXL_QUEUE: a job) in batch row b, whose logits row it draws from and whose
// next input it writes, after emo_grammar_open has brought the stream's words to sst / spr and found it RUNNING.  All 512 threads call it; every
// barrier inside lies on a path that sst, spr and the launch arguments alone decide.  CTL: the block has sampling controls (emo_grammar_controls).
// GUIDE (kind TXL alone): the block has the three guidance tables; a stream whose pair (guide_cond[r], guide_uncond[r]) is two distinct rows of
// the batch draws from their combination (emo_guided_logits) with the uniforms and the controls of row guide_cond[r], every other stream as
// without them.  The pair is the same word in every thread, so the barriers stay uniform.  The scores are still taken from the stream's own row b.
// KEEP: the block has the kept-bar tables; skl[0] is keep_left[r] as emo_grammar_open's barrier published it (read by every thread, written in
// memory by thread 0 alone, like the state words).
template <bool CTL, bool GUIDE, bool KEEP>
__device__ __forceinline__ void txl_stream_step(const emo_grammar_step_t& a, int64_t b, int64_t r, char* lds, const int32_t* sst, const int32_t* spr,
                                                const int32_t* skl, int32_t* sacc, float* sred, int tid) {
    int32_t* st = a.state + r * EMO_TXL_STATE_WORDS;
    int64_t* row = a.seq + r * a.ld_seq;
    const int32_t plen = spr[EMO_TXL_P_PRIMER_LEN];
    if (sst[EMO_TXL_S_FEED] < plen) {
        if (tid == 0) {
            a.tok_out[b] = row[sst[EMO_TXL_S_FEED]];
            st[EMO_TXL_S_FEED] = sst[EMO_TXL_S_FEED] + 1;
        }
        return;
    }
    if constexpr (KEEP) {
        const int32_t left = skl[0];
        if (left > 0 && left <= sst[EMO_TXL_S_LEN]) {        // a kept token written behind an accepted Bar is fed: no draw
            if (tid == 0) {
                a.tok_out[b] = row[sst[EMO_TXL_S_LEN] - left];
                a.keep_left[r] = left - 1;
            }
            return;
        }
    }
    const int32_t draws = sst[EMO_TXL_S_DRAWS];
    if (draws >= a.n_u) {                                    // the caller's uniform table is exhausted: the stream stops with an error status
        if (tid == 0) {
            st[EMO_TXL_S_STATUS] = EMO_TXL_OVERFLOW;
            atomicSub(a.running, 1);
        }
        return;
    }
    const int32_t len = sst[EMO_TXL_S_LEN];
    const bool key_step = spr[EMO_TXL_P_KEYED] != 0 && len == 1;          // the event after the emotion tag is the key (:81-89)
    int64_t word;
    // (the key draw keeps key_temperature / key_top_p; the ban, the bias and the two cuts hold for it too)
    if constexpr (GUIDE) {
        const int64_t gc = a.guide_cond[r], gu = a.guide_uncond[r];
        if (gc != gu && gc >= 0 && gc < a.n_rows && gu >= 0 && gu < a.n_rows) {
            const emo_grammar_controls_t ctl = emo_grammar_controls<CTL>(a, gc);
            word = emo_nucleus_draw_from(emo_guided_logits{a.logits + gc * a.n_token, a.logits + gu * a.n_token, a.guide_scale[r], ctl.ban, ctl.bias},
                                         a.n_token, key_step ? a.key_temperature : ctl.temp, key_step ? a.key_top_p : ctl.top_p, ctl.top_k, ctl.min_p,
                                         a.u_steps[(int64_t)draws * a.ld_u + gc], lds, tid, [] { __syncthreads(); });
        } else {
            const emo_grammar_controls_t ctl = emo_grammar_controls<CTL>(a, r);
            word = emo_nucleus_draw_from(emo_banned_logits{a.logits + b * a.n_token, ctl.ban, ctl.bias}, a.n_token, key_step ? a.key_temperature : ctl.temp,
                                         key_step ? a.key_top_p : ctl.top_p, ctl.top_k, ctl.min_p, a.u_steps[(int64_t)draws * a.ld_u + r], lds, tid,
                                         [] { __syncthreads(); });
        }
    } else {
        const emo_grammar_controls_t ctl = emo_grammar_controls<CTL>(a, r);
        word = emo_nucleus_draw_from(emo_banned_logits{a.logits + b * a.n_token, ctl.ban, ctl.bias}, a.n_token, key_step ? a.key_temperature : ctl.temp,
                                     key_step ? a.key_top_p : ctl.top_p, ctl.top_k, ctl.min_p, a.u_steps[(int64_t)draws * a.ld_u + r], lds, tid,
                                     [] { __syncthreads(); });
    }
    if (!emo_grammar_wants_scores(a)) {
        if (tid == 0) txl_grammar<KEEP>(a, b, r, row, st, sst, spr, word, draws, key_step, len);
        return;
    }
    if (tid == 0) {
        sacc[0] = txl_grammar<KEEP>(a, b, r, row, st, sst, spr, word, draws, key_step, len);
        sacc[1] = (int32_t)word;
    }
    __syncthreads();
    if (sacc[0] >= 0) emo_grammar_score(a, a.logits + b * a.n_token, r, sacc[0], sacc[1], sred, tid);
}

template <bool CTL, bool GUIDE, bool KEEP>
__global__ __launch_bounds__(512) void txl_grammar_kernel(const emo_grammar_step_t a) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_TXL_STATE_WORDS], spr[EMO_TXL_PARAM_WORDS];
    __shared__ int32_t sacc[KEEP ? 3 : 2];                     // (KEEP: the third word is keep_left[r]; without the tables the array of before)
    __shared__ float sred[EMO_DRAW_SCORES_WORDS];
    int32_t* const skl = sacc + 2;
    const int tid = (int)threadIdx.x;
    const int64_t r = blockIdx.x;
    if constexpr (KEEP) {
        if (tid == 16) skl[0] = a.keep_left[r];              // published by the barrier of emo_grammar_open
    }
    emo_grammar_open(a.state + r * EMO_TXL_STATE_WORDS, EMO_TXL_STATE_WORDS, a.params + r * EMO_TXL_PARAM_WORDS, EMO_TXL_PARAM_WORDS, sst, spr, tid);
    if (sst[EMO_TXL_S_STATUS] != EMO_TXL_RUNNING) return;
    txl_stream_step<CTL, GUIDE, KEEP>(a, r, r, lds, sst, spr, skl, sacc, sred, tid);
}

// Thread 0 of slot b, whose job (if it had one) is over: the next queued job that is RUNNING, or none.  queue_head only grows, so a slot that
// has seen it at n_jobs never adds to it again.
__device__ __forceinline__ void txl_queue_admit(const emo_grammar_step_t& a, int64_t b) {
    int32_t next = -1;
    while (__atomic_load_n(a.queue_head, __ATOMIC_RELAXED) < a.n_jobs) {
        const int32_t h = atomicAdd(a.queue_head, 1);
        if (h >= a.n_jobs) break;
        if (a.state[(int64_t)h * EMO_TXL_STATE_WORDS + EMO_TXL_S_STATUS] == EMO_TXL_RUNNING) {      // (a job closed on the host is passed over)
            next = h;
            break;
        }
    }
    a.slot_job[b] = next;
    a.mem_lens[b] = 0;                                       // the row of the model's memory starts again; a free slot stays at row 0
    if (next >= 0) {
        a.tok_out[b] = a.seq[(int64_t)next * a.ld_seq];      // the model step behind this launch is the new job's first token
        a.state[(int64_t)next * EMO_TXL_STATE_WORDS + EMO_TXL_S_FEED] = 1;
    }
}

template <bool CTL, bool KEEP>
__global__ __launch_bounds__(512) void txl_queue_kernel(const emo_grammar_step_t a) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_TXL_STATE_WORDS], spr[EMO_TXL_PARAM_WORDS];
    __shared__ int32_t sacc[KEEP ? 3 : 2], sslot[2];           // (KEEP: the third word is keep_left[j]; without the tables the array of before)
    __shared__ float sred[EMO_DRAW_SCORES_WORDS];
    int32_t* const skl = sacc + 2;
    const int tid = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid == 0) {                                          // thread 0 writes slot_job[b] and mem_lens[b] below: the others decide from this copy
        sslot[0] = a.slot_job[b];
        sslot[1] = a.mem_lens[b] >= a.mem_rows;
    }
    __syncthreads();
    const int64_t j = sslot[0];
    if (j < 0 || j >= a.n_jobs) {                            // a free slot
        if (tid == 0) txl_queue_admit(a, b);
        return;
    }
    int32_t* st = a.state + j * EMO_TXL_STATE_WORDS;
    if constexpr (KEEP) {
        if (tid == 16) skl[0] = a.keep_left[j];              // per job; published by the barrier of emo_grammar_open
    }
    emo_grammar_open(st, EMO_TXL_STATE_WORDS, a.params + j * EMO_TXL_PARAM_WORDS, EMO_TXL_PARAM_WORDS, sst, spr, tid);
    if (sst[EMO_TXL_S_STATUS] == EMO_TXL_RUNNING) {
        if (sslot[1]) {                                      // the row has no place for another token
            if (tid == 0) {
                st[EMO_TXL_S_STATUS] = EMO_TXL_MEM_FULL;
                atomicSub(a.running, 1);
            }
        } else {
            txl_stream_step<CTL, false, KEEP>(a, b, j, lds, sst, spr, skl, sacc, sred, tid);      // (the queue kind ignores the guidance tables)
        }
    }
    if (tid == 0 && st[EMO_TXL_S_STATUS] != EMO_TXL_RUNNING) {      // (thread 0 reads what it wrote itself)
        if (a.job_steps) a.job_steps[j] = (int32_t)a.mem_lens[b];    // tokens the model was fed for the job = launches it held the slot
        txl_queue_admit(a, b);
    }
}

}  // namespace

// (a block without the guidance tables launches a <.., false, ..> instance, a block without the kept-bar tables a <.., false> one: the kernels
// as they were before either existed; emo_grammar_step has checked that each set comes together)
int emo_txl_grammar_launch(const emo_grammar_step_t& a, emo_stream_t stream) {
    const bool ctl = emo_grammar_has_controls(a), guide = a.guide_cond != nullptr, keep = a.keep_tok != nullptr;
    const auto kernel = keep    ? (guide ? (ctl ? txl_grammar_kernel<true, true, true> : txl_grammar_kernel<false, true, true>)
                                         : (ctl ? txl_grammar_kernel<true, false, true> : txl_grammar_kernel<false, false, true>))
                        : guide ? (ctl ? txl_grammar_kernel<true, true, false> : txl_grammar_kernel<false, true, false>)
                                : (ctl ? txl_grammar_kernel<true, false, false> : txl_grammar_kernel<false, false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.n_rows), dim3(512), 0, (hipStream_t)stream, a);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}

int emo_txl_queue_launch(const emo_grammar_step_t& a, emo_stream_t stream) {
    const bool ctl = emo_grammar_has_controls(a), keep = a.keep_tok != nullptr;
    const auto kernel = keep ? (ctl ? txl_queue_kernel<true, true> : txl_queue_kernel<false, true>)
                             : (ctl ? txl_queue_kernel<true, false> : txl_queue_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.n_rows), dim3(512), 0, (hipStream_t)stream, a);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
