// Stage-1 lead-sheet generation: the sample-and-grammar half of one lock-step token step (reference stage1_compose/inference_utils.py:51-134,
// match_emotion_key :137-142).  One 512-thread workgroup per stream; all loop state lives in device memory (no allocation, graph-capturable).
// The draw is emo_nucleus_draw, the device code of emo_sample_nucleus, so a stream picks the same id from the same logits and uniform.
// Per stream r:
//   finished            -> nothing;
//   feeding the primer  -> tok_out[r] = seq[r, feed], feed += 1, no draw (a primer longer than the common prefix, or a re-fed primer);
//   otherwise           -> draw with u_steps[draws, r], run the grammar in the reference's order (key rule, Beat, Bar, PAD, append, end tests)
//                          and choose the next input: the accepted word, the previous input again after a rejection, or — when nothing has
//                          been accepted yet — the whole primer again from its first token (the reference re-submits `generated`).
#include "emo_nucleus.h"

namespace {

__global__ __launch_bounds__(512) void txl_grammar_kernel(const float* __restrict__ logits, int64_t n, int64_t V, float temp, float top_p,
                                                          float key_temp, float key_top_p, const float* __restrict__ u_steps, int64_t n_u,
                                                          const int32_t* __restrict__ ev_flags, const int32_t* __restrict__ ev_beat,
                                                          const int32_t* __restrict__ params, int32_t* __restrict__ state, int64_t* __restrict__ seq,
                                                          int64_t ld_seq, int64_t* __restrict__ tok_out, int32_t* __restrict__ running) {
    __shared__ __attribute__((aligned(16))) char lds[EMO_NUCLEUS_LDS];
    __shared__ int32_t sst[EMO_TXL_STATE_WORDS], spr[EMO_TXL_PARAM_WORDS];
    const int tid = (int)threadIdx.x;
    const int64_t r = blockIdx.x;
    int32_t* st = state + r * EMO_TXL_STATE_WORDS;
    int64_t* row = seq + r * ld_seq;
    // thread 0 alone touches the stream's state in memory: the other threads decide from this copy, so a write below can never change the
    // path (and the barrier count) of a thread that has not read yet
    if (tid < EMO_TXL_STATE_WORDS) sst[tid] = st[tid];
    if (tid < EMO_TXL_PARAM_WORDS) spr[tid] = params[r * EMO_TXL_PARAM_WORDS + tid];
    __syncthreads();
    if (sst[EMO_TXL_S_STATUS] != EMO_TXL_RUNNING) return;
    const int32_t plen = spr[EMO_TXL_P_PRIMER_LEN];
    if (sst[EMO_TXL_S_FEED] < plen) {
        if (tid == 0) {
            tok_out[r] = row[sst[EMO_TXL_S_FEED]];
            st[EMO_TXL_S_FEED] = sst[EMO_TXL_S_FEED] + 1;
        }
        return;
    }
    const int32_t draws = sst[EMO_TXL_S_DRAWS];
    if (draws >= n_u) {                                      // the caller's uniform table is exhausted: the stream stops with an error status
        if (tid == 0) {
            st[EMO_TXL_S_STATUS] = EMO_TXL_OVERFLOW;
            atomicSub(running, 1);
        }
        return;
    }
    int32_t len = sst[EMO_TXL_S_LEN];
    const bool key_step = spr[EMO_TXL_P_KEYED] != 0 && len == 1;          // the event after the emotion tag is the key (:81-89)
    const int64_t word = emo_nucleus_draw(logits + r * V, V, key_step ? key_temp : temp, key_step ? key_top_p : top_p, u_steps[(int64_t)draws * n + r],
                                          lds, tid, [] { __syncthreads(); });
    if (tid != 0) return;
    const int32_t fl = ev_flags[word];
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
            const int32_t pos = ev_beat[word];
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
            } else if (len >= ld_seq) {
                status = EMO_TXL_OVERFLOW;
            } else {
                row[len++] = word;
                ++accepted;
                if (len > spr[EMO_TXL_P_MAX_EVENTS] || (fl & EMO_TXL_EV_EOS)) status = EMO_TXL_DONE;
            }
        }
    }
    if (status == EMO_TXL_RUNNING && bars >= spr[EMO_TXL_P_MAX_BARS]) status = EMO_TXL_DONE;
    if (status == EMO_TXL_RUNNING && accepted == 0) {
        tok_out[r] = row[0];                                 // nothing accepted yet: the whole primer again, one token per step
        feed = 1;
    } else {
        tok_out[r] = row[len - 1];                           // the accepted word, or after a rejection the previous input again (a finished
    }                                                        // stream's row idles on its last token)
    st[EMO_TXL_S_STATUS] = status;
    st[EMO_TXL_S_LEN] = len;
    st[EMO_TXL_S_ACCEPTED] = accepted;
    st[EMO_TXL_S_BEAT] = beat;
    st[EMO_TXL_S_BARS] = bars;
    st[EMO_TXL_S_FAILED] = failed;
    st[EMO_TXL_S_FEED] = feed;
    st[EMO_TXL_S_DRAWS] = draws + 1;
    if (status != EMO_TXL_RUNNING) atomicSub(running, 1);
}

}  // namespace

extern "C" int emo_txl_grammar_step(const float* logits, int64_t n, int64_t V, float temperature, float top_p, float key_temperature, float key_top_p,
                                    const float* u_steps, int64_t n_u, const int32_t* ev_flags, const int32_t* ev_beat, const int32_t* params,
                                    int32_t* state, int64_t* seq, int64_t ld_seq, int64_t* tok_out, int32_t* running, emo_stream_t stream) {
    EMO_CHECK(logits && u_steps && ev_flags && ev_beat && params && state && seq && tok_out && running, "emo_txl_grammar_step: null pointer");
    EMO_CHECK(n > 0 && n_u > 0 && ld_seq > 0, "emo_txl_grammar_step: bad sizes");
    EMO_CHECK(V > 0 && V <= 1024, "emo_txl_grammar_step: V must be <= 1024 (got %lld)", (long long)V);
    EMO_CHECK(temperature > 0.f && key_temperature > 0.f, "emo_txl_grammar_step: temperatures must be > 0");
    hipLaunchKernelGGL(txl_grammar_kernel, dim3((unsigned)n), dim3(512), 0, (hipStream_t)stream, logits, n, V, temperature, top_p, key_temperature,
                       key_top_p, u_steps, n_u, ev_flags, ev_beat, params, state, seq, ld_seq, tok_out, running);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
