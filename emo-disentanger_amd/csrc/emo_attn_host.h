// Host glue of the attention files (emo_favor*.hip, emo_softmax_attn*.hip): the launchers below emo_attn read the argument block emo_attn_t
// themselves and take, next to it, only what is derived from it (the DropCtx, the FAVOR segment geometry, the stage, the stream).
#pragma once
#include <stdlib.h>

#include "emo_common.h"

// ---------------------------------------------------------------- switches
// Read from the environment on EVERY call and never cached: tests toggle EMO_FAVOR_FS, EMO_SATTN32, ... in-process.
static inline int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}
static inline bool env_off(const char* name) { return env_int(name, 1) == 0; }   // NAME=0 switches a path off; unset or anything else leaves it on

// ---------------------------------------------------------------- launch
// One launch of the kernel instance `Kernel`.  Its dynamic-LDS limit is raised to lds_max before the instance's first launch in the process and
// never again (lds_max = 0: the instance uses no dynamic LDS and the attribute is left alone); a failed launch returns EMO_ERR_LAUNCH with
// EMO_LAUNCH_CHECK's message.
#define EMO_TRY(...)                              \
    do {                                          \
        const int rc__ = (__VA_ARGS__);           \
        if (rc__ != EMO_OK) return rc__;          \
    } while (0)
template <auto Kernel, typename... Args>
static int emo_launch_lds(dim3 grid, dim3 block, size_t lds_max, size_t lds, hipStream_t st, Args... args) {
    static bool attr = false;
    if (!attr) {
        if (lds_max) (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        attr = true;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    EMO_LAUNCH_CHECK();
    return EMO_OK;
}
// (the instances whose LDS size is a constant of the instance: the limit is what every launch asks for)
template <auto Kernel, typename... Args> static int emo_launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    return emo_launch_lds<Kernel>(grid, block, lds, lds, st, args...);
}

// ---------------------------------------------------------------- dtype x d_head
// attn_by_dtype<F>(a, ...) = F::run<CT>(a, ...) with CT the element type of a.dtype (the entry has checked it to be EMO_F32 or EMO_BF16): the
// decode passes of SOFTMAX and RELPOS, whose kernels take d_head at run time.  attn_by_dtype_dh<F>(a, ...) = F::run<CT, DH>(a, ...) over the
// d_head instances built for the training passes of both kinds.  (FAVOR keeps its own (d_head, n_feat) table, emo_favor.hip.)
template <typename F, typename... A> static int attn_by_dtype(const emo_attn_t& a, A... args) {
    return a.dtype == EMO_BF16 ? F::template run<bf16_t>(a, args...) : F::template run<float>(a, args...);
}
template <typename F> struct AttnByDh {
    template <typename CT, typename... A> static int run(const emo_attn_t& a, A... args) {
        if (a.dh == 64) return F::template run<CT, 64>(a, args...);
        if (a.dh == 32) return F::template run<CT, 32>(a, args...);
        if (a.dh == 16) return F::template run<CT, 16>(a, args...);
        emo_set_error("unsupported d_head=%lld (built: 16, 32, 64)", (long long)a.dh);
        return EMO_ERR_UNSUPPORTED;
    }
};
template <typename F, typename... A> static int attn_by_dtype_dh(const emo_attn_t& a, A... args) { return attn_by_dtype<AttnByDh<F>>(a, args...); }

// ---------------------------------------------------------------- the kernels of the other file of a kind
// Each *_try returns 1 when it served the call, 0 when the shape, the alignment or a switch leaves it to the caller's generic kernels, and a
// negative EMO_ERR_* when its launch failed.
// emo_favor_fs.hip: the bf16 / d_head 64 / 128-feature "slice" kernels.  stage: the whole forward, or one main pass of the backward.  P > 1: the
// caller has run the generic state-only pass into ws_S / ws_z — the K-state increments before DQ, the R-state increments before DKV.
enum favor_stage_t { FAVOR_STAGE_FWD, FAVOR_STAGE_DQ, FAVOR_STAGE_DKV };
int emo_favor_fs_try(const emo_attn_t& a, favor_stage_t stage, int P, int64_t Ts, const float* ws_S, const float* ws_z, hipStream_t st);
// emo_softmax_attn32.hip: bf16 / d_head 64 / T % 128 == 0 kernels on 32 x 32 x 16 tiles, one function per pass (the dQ pass writes delta_ws for the
// dK / dV pass); and the bytes of the keep words of one call (0: these kernels do not serve the shape, or dropout is off)
int emo_sattn32_fwd_try(const emo_attn_t& a, DropCtx drop, hipStream_t st);
int emo_sattn32_dq_try(const emo_attn_t& a, DropCtx drop, hipStream_t st);
int emo_sattn32_dkv_try(const emo_attn_t& a, DropCtx drop, hipStream_t st);
int64_t emo_sattn32_keep_bytes(int64_t B, int64_t T, int64_t H, int64_t dh, float p_drop);
