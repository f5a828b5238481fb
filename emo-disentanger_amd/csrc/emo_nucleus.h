// Nucleus (top-p) draw of ONE stream by 512 threads — shared by nucleus_kernel (emo_elementwise.hip) and the one-launch decode step
// (emo_decode_persist.hip), which must pick the same token from the same logits bit for bit.  Reference: stage2_accompaniment/inference.py:71-100.
// probs = softmax(l/temp) (fp32, as NumPy on fp32 logits); rank sort (descending, ties by ascending index) of <= 1024 entries in LDS; inclusive
// cumsum in np.cumsum's sequential fp32 order; last_index = SECOND position whose cumsum exceeds top_p (the reference keeps the crossing token —
// SURVEY F12); where the reference would raise IndexError (single crossing) all sorted tokens are kept; no crossing keeps the top min(V, 3).  Draw:
// cdf over the renormalised (f64) candidates, searchsorted(u, right).
// Ascending index among EQUAL probabilities is THIS PROJECT's rule, not the reference's: the reference's order among exact ties is whatever NumPy's
// unstable argsort produces (on tests/golden/sampling.json neither ascending nor descending index), so a tie group that straddles the cut keeps
// its lowest indices here and an arbitrary subset of the same size there.  tests/test_gpu_sampling.py pins the rule and holds this header to a
// float64 restatement (tests/nucleus_ref.py) with derived rounding bounds.
// The logits are read through an accessor (emo_nucleus_draw_from): emo_plain_logits is the load itself, emo_banned_logits reads a banned token's
// logit as -INFINITY and leaves the arithmetic alone, so a draw under a ban is bit for bit the plain draw from a row overwritten that way;
// emo_guided_logits combines two rows (classifier-free guidance), bit for bit the plain draw from the row a float32 host combination writes.
// Both take an optional additive bias row (NULL: the accessor as it was): l(c) + bias[c], ONE rounded fp32 add behind the combination and in
// front of the ban, bit for bit the plain draw from the row NumPy's float32 `l + b` writes; a bias of -inf is a ban.
// Two optional cuts narrow the candidate count behind top-p's (emo_nucleus_pick): top_k (a rank cap; <= 0: off) and min_p (a floor relative to
// the best probability; <= 0: off).  Both are counts over the sorted arrays, so the tie rule above holds for them: a tie group that straddles
// top_k keeps its lowest indices.  sampling.soft_cut_count restates them on the host.
#pragma once
#include "emo_common.h"

constexpr int EMO_NUCLEUS_LDS = (3 * (1024 + 8)) * 4 + (1024 + 8) * 8 * 2 + 1024 * 4 + 64;      // bytes of LDS scratch (16-B aligned base)
constexpr int EMO_NUCLEUS_BARRIERS = 9;                                                          // sync() calls of emo_nucleus_draw (every path, with or without the two cuts)

// The candidate cut and the draw of emo_nucleus_draw, from the sorted probabilities and prefixes it leaves in LDS: a second draw from the same
// logits with another uniform costs only this part (3 barriers).  Same contract as emo_nucleus_draw: the id in thread 0.
// The candidate count is min(last, top_k, n_m): `last` as top-p gives it with all its edge rules; top_k <= 0 is off (top_k >= V changes
// nothing); n_m = max(1, #{i < V : sp[i] >= min_p * sp[0]}) over the sorted fp32 probabilities, the product ONE rounded fp32 multiply, min_p <= 0
// (or NaN) off.  n_m is counted in the pass that counts the first crossing and travels in the upper half of the same LDS word (both counts are
// <= 1024), so the cuts add no barrier; with both off (constants in the callers that have no controls) the code is the one without them.  The
// f64 renormalisation and the draw run over the final count.
template <typename Sync>
__device__ __forceinline__ int64_t emo_nucleus_pick(int64_t V, float top_p, int top_k, float min_p, float u, char* lds, int tid, Sync sync) {
    float* sp = (float*)lds;
    float* sq = sp + 1024 + 8;
    float* cumf = sq + 1024 + 8;
    double* cumd = (double*)(cumf + 1024 + 8);
    unsigned long long* skey = (unsigned long long*)(cumd + 1024 + 8);
    int* si = (int*)(skey + 1024 + 8);
    float* red = (float*)(si + 1024);
    int* cnt = (int*)(red + 8);
    const int lane = tid & 63, wave = tid >> 6;
    // first crossing i1 = #{i < V : cum_i <= top_p}; cum is non-decreasing, so the second crossing is i1 + 1
    const bool floor_on = min_p > 0.f;
    int c1 = 0;
    if (floor_on) {
#pragma clang fp contract(off)
        const float thr = min_p * sp[0];                       // one rounded multiply (the pragma covers this block alone)
        int cm = 0;
        for (int i = tid; i < V; i += 512) {
            c1 += (cumf[i] <= top_p) ? 1 : 0;
            cm += (sp[i] >= thr) ? 1 : 0;
        }
        c1 = (int)wave_sum((float)c1);
        cm = (int)wave_sum((float)cm);
        if (lane == 0) cnt[wave] = c1 | (cm << 16);
    } else {
        for (int i = tid; i < V; i += 512) c1 += (cumf[i] <= top_p) ? 1 : 0;
        c1 = (int)wave_sum((float)c1);
        if (lane == 0) cnt[wave] = c1;
    }
    sync();
    const int both = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + cnt[5] + cnt[6] + cnt[7];
    const int i1 = floor_on ? (both & 0xFFFF) : both;
    int last;
    if (i1 >= V) last = V < 3 ? (int)V : 3;       // no crossing
    else if (i1 + 1 >= V) last = (int)V;          // single crossing (reference: IndexError)
    else last = i1 + 1;
    if (top_k > 0 && top_k < last) last = top_k;
    if (floor_on) {
        const int n_m = (both >> 16) > 0 ? (both >> 16) : 1;
        if (n_m < last) last = n_m;
    }
    const double target = (double)u * cumd[last - 1];
    sync();
    int c2 = 0;
    for (int i = tid; i < last; i += 512) c2 += (cumd[i] <= target) ? 1 : 0;
    c2 = (int)wave_sum((float)c2);
    if (lane == 0) cnt[wave] = c2;
    sync();
    int64_t tok = 0;
    if (tid == 0) {
        int pick = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + cnt[5] + cnt[6] + cnt[7];
        if (pick >= last) pick = last - 1;
        tok = (int64_t)si[pick];
    }
    return tok;
}

// The logit accessors of the draw: l(c) = the logit of token c, c in [0, V).
struct emo_plain_logits {
    const float* __restrict__ row;
    __device__ __forceinline__ float operator()(int c) const { return row[c]; }
};
// `ban` (NULL: no ban, the plain load): uint32 words, bit c & 31 of word c >> 5 set = token c is banned.  Only bits of c < V are ever read.
// `bias` (NULL: none): f32 [V], added to the logit with one rounded fp32 add; the ban is applied last.
struct emo_banned_logits {
    const float* __restrict__ row;
    const uint32_t* __restrict__ ban;
    const float* __restrict__ bias = nullptr;
    __device__ __forceinline__ float operator()(int c) const {
        if (ban && ((ban[c >> 5] >> (c & 31)) & 1u)) return -INFINITY;
        const float lc = row[c];
        if (bias) {
#pragma clang fp contract(off)
            return lc + bias[c];                                 // one rounded add, never fused into the division behind it
        }
        return lc;
    }
};
// Classifier-free guidance: l(c) = lc + s * (lc - lu) over a conditioned and an unconditioned row, as __fadd_rn(lc, __fmul_rn(s, __fsub_rn(lc,
// lu))): THREE separately rounded fp32 operations.  Those intrinsics are plain operators in this toolchain, which the default contraction may
// fuse after inlining, so the operators stand here themselves with contraction switched off: NumPy's float32 `lc + s * (lc - lu)` is then the
// same row bit for bit.  The ban is applied after the combination (no inf - inf arises from it); s = 0 is the conditioned row itself.
// `bias` (NULL: none) is added AFTER the three operations, a fourth separately rounded one: NumPy's float32 `(lc + s * (lc - lu)) + b`.
struct emo_guided_logits {
    const float* __restrict__ cond;
    const float* __restrict__ uncond;
    float scale;
    const uint32_t* __restrict__ ban;
    const float* __restrict__ bias = nullptr;
    __device__ __forceinline__ float operator()(int c) const {
#pragma clang fp contract(off)
        if (ban && ((ban[c >> 5] >> (c & 31)) & 1u)) return -INFINITY;
        const float lc = cond[c];
        const float d = lc - uncond[c];
        const float m = scale * d;
        const float g = lc + m;
        return bias ? g + bias[c] : g;
    }
};

// tid in [0, 512); `sync` = a barrier over exactly the calling threads (+ any others that call it the same number of times).  Returns the picked
// token id in thread 0 (other threads: undefined).  u = the uniform draw of this stream; top_k / min_p: the two cuts of emo_nucleus_pick.
template <typename Logits, typename Sync>
__device__ __forceinline__ int64_t emo_nucleus_draw_from(const Logits l, int64_t V, float temp, float top_p, int top_k, float min_p, float u, char* lds,
                                                         int tid, Sync sync) {
    float* sp = (float*)lds;
    float* sq = sp + 1024 + 8;
    float* cumf = sq + 1024 + 8;
    double* cumd = (double*)(cumf + 1024 + 8);
    unsigned long long* skey = (unsigned long long*)(cumd + 1024 + 8);
    int* si = (int*)(skey + 1024 + 8);
    float* red = (float*)(si + 1024);
    const int Vp = ((int)V + 7) & ~7;
    const int lane = tid & 63, wave = tid >> 6;
    float mx = -INFINITY;
    for (int c = tid; c < V; c += 512) mx = fmaxf(mx, l(c) / temp);
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    sync();
    mx = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
    sync();
    float s = 0.f;
    for (int c = tid; c < V; c += 512) {
        const float e = expf(l(c) / temp - mx);
        sp[c] = e;
        s += e;
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    sync();
    const float tot = red[0] + red[1] + red[2] + red[3] + red[4] + red[5] + red[6] + red[7];
    // rank sort on 64-bit keys {probability bits, ~index}: key_j > key_c  <=>  p_j > p_c, or p_j == p_c and j < c (probabilities are >= 0, so their
    // bit patterns order like their values) - a total order (the tie rule above) in ONE compare + ONE add-with-carry per pair
    // (r04: the float version spent ~7 VALU instructions per pair, 336 x 336 pairs on 6 waves = half of the kernel's 20 us).  Pad keys are 0.
    for (int c = tid; c < V; c += 512) {
        const float pc = sp[c] / tot;
        sq[c] = pc;
        skey[c] = ((unsigned long long)__builtin_bit_cast(unsigned, pc) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c);
    }
    for (int c = (int)V + tid; c < Vp + 8; c += 512) { sq[c] = -1.f; skey[c] = 0ull; }
    sync();
    for (int c = tid; c < Vp; c += 512) {
        if (c < V) {
            const float pc = sq[c];
            const unsigned long long kc = skey[c];
            int rank = 0;
            for (int j0 = 0; j0 < Vp; j0 += 2) {
                const u32x4 k2 = *(const u32x4*)(skey + j0);
                const unsigned long long ka = ((unsigned long long)k2[1] << 32) | k2[0], kb = ((unsigned long long)k2[3] << 32) | k2[2];
                rank += (int)(ka > kc) + (int)(kb > kc);
            }
            sp[rank] = pc;
            si[rank] = c;
        } else {
            sp[c] = 0.f;                                                   // sorted tail pad: adds nothing to either prefix
        }
    }
    sync();
    // Both prefixes stay SEQUENTIAL (np.cumsum order: the top-p crossing and the draw are rounding-sensitive), but a chunk of 32 sorted values is
    // fetched into registers before its dependent chain of adds runs (r04: the loops used to pay an LDS round trip per 4-8 values, and the f64 one
    // was ~9 of the kernel's 20 us).
    if (tid == 0) {                        // np.cumsum order, fp32
        float cum = 0.f;
        for (int i0 = 0; i0 < Vp; i0 += 32) {
            f32x4 a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = (i0 + 4 * j < Vp) ? *(const f32x4*)(sp + i0 + 4 * j) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                f32x4 ca;
                ca[0] = cum += a[j][0]; ca[1] = cum += a[j][1]; ca[2] = cum += a[j][2]; ca[3] = cum += a[j][3];
                if (i0 + 4 * j < Vp) *(f32x4*)(cumf + i0 + 4 * j) = ca;
            }
        }
    } else if (tid == 64) {                // sequential f64 prefix of the same sorted probabilities (candidate renormalisation + draw)
        double run = 0.0;
        for (int i0 = 0; i0 < Vp; i0 += 32) {
            f32x4 a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = (i0 + 4 * j < Vp) ? *(const f32x4*)(sp + i0 + 4 * j) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                double c0, c1, c2, c3;
                c0 = run += (double)a[j][0]; c1 = run += (double)a[j][1]; c2 = run += (double)a[j][2]; c3 = run += (double)a[j][3];
                if (i0 + 4 * j < Vp) { cumd[i0 + 4 * j] = c0; cumd[i0 + 4 * j + 1] = c1; cumd[i0 + 4 * j + 2] = c2; cumd[i0 + 4 * j + 3] = c3; }
            }
        }
    }
    sync();
    return emo_nucleus_pick(V, top_p, top_k, min_p, u, lds, tid, sync);
}

// The draw from a plain row of logits, both cuts off: nucleus_kernel and the sampled one-launch decode step.
template <typename Sync>
__device__ __forceinline__ int64_t emo_nucleus_draw(const float* __restrict__ l, int64_t V, float temp, float top_p, float u, char* lds, int tid, Sync sync) {
    return emo_nucleus_draw_from(emo_plain_logits{l}, V, temp, top_p, 0, 0.f, u, lds, tid, sync);
}
