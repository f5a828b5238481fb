// Which kernel serves an emo_gemm call, and how: ONE pure function of the call's arguments and the EMO_* switches (host only: no HIP, no operand
// is dereferenced, no thread-local is written).  emo_gemm executes the plan, emo_gemm_route reports it, emo_gemm_workspace_bytes sizes from it.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "emo_hip.h"
// ------------------------------------------------------------------------------------------------ tile geometry the gates depend on
// (the kernel files static_assert their own constants against these)
constexpr int GP_BM = 128, GP_BN = 128, GP_BK = 64, GP_RING_BK = 32;          // 128 x 128 tile: register-staged K step, K granularity of the LDS-DMA ring
constexpr int GP_AS_K = 512, GP_AS_BM = 128, GP_AS_BN = 64, GP_AS_KS = 128, GP_AS_MAXN = 2048, GP_AS_MIN_BLOCKS = 32;   // A-stationary: below one panel per CU the columns are split
constexpr int GP_W_BM = 256, GP_W_BN = 256, GP_W_BK = 64, GP_W_STAGES = 3;    // 256 x 256 tile (NT and wgrad)
constexpr int GP_MAX_SPLITS = 32;                                             // K-splits emo_gemm_workspace_bytes sizes the plain split-K for
// A-stationary kernel instances (template argument = epilogue feature flags)
enum { AF_RELU = 1, AF_DROP = 2, AF_RES = 4, AF_BITS = 8, AF_MASKOUT = 16, AF_GENERIC = 32, AF_DGELU = 64, AF_GELUAUX = 128, AF_HDIV = 256 };   // (DGELU, GELUAUX: GPT-2's MLP; HDIV: emo_hip.h hdiv)
static inline int64_t gp_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// ------------------------------------------------------------------------------------------------ the switches, all of them, read here only
// Read per call (tests toggle them in-process) unless marked latched.
static inline int gp_env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
static inline int64_t gp_env_pos(const char* name, int64_t unset) { const char* e = getenv(name); return (e && atoll(e) > 0) ? atoll(e) : unset; }     // (values <= 0: unset)
// EMO_GEMM_SAFE_TR=1 (latched at first use): scalar LDS reads instead of the transposing read; only the register-staged kernel has them
inline bool gp_safe_tr() { static const bool on = [] { const char* e = getenv("EMO_GEMM_SAFE_TR"); return e && e[0] == '1'; }(); return on; }
// EMO_GEMM_VARIANT (latched): 1 = register-staged v1, 2 = LDS-DMA ring for k-contiguous A, 3 = also for the TN (wgrad) layout; unset = per call (r05):
// the weight-gradient layout (A stored [K, M]) on the LDS-DMA kernel when the reduction is short — stage 1 (2048 tokens per step: 48 weight gradients on the
// register-staged kernel) 6.35 -> 6.13 ms per step; at 8192 tokens it measures the same, at 131072 it loses 1.5 ms (those shapes have the 256 x 256 wgrad
// kernel; what reaches the 128 x 128 tiles then is better off with the in-kernel bias gradient of v1).
inline int gp_variant(int a_trans, int64_t K) {
    static const int forced = [] { const char* e = getenv("EMO_GEMM_VARIANT"); return (e && e[0] >= '1' && e[0] <= '3') ? e[0] - '0' : 0; }();
    return forced ? forced : ((a_trans && K <= 4096) ? 3 : 2);
}
inline bool gp_small_grid_ring() { static const bool on = gp_env_int("EMO_GEMM_SMALLGRID", 1) != 0; return on; }     // (latched)
inline bool gp_small_grid_bk64() { static const bool on = gp_env_int("EMO_GEMM_SMALL64", 1) != 0; return on; }       // (latched) 0: the 32-deep ring
static inline int64_t gp_astat_min_rows() { return gp_env_pos("EMO_ASTAT_MIN_ROWS", (int64_t)GP_AS_BM * GP_AS_MIN_BLOCKS); }      // (A/B of the column split)
// ------------------------------------------------------------------------------------------------ the call, as far as routing looks at it
struct GemmCall {
    int a_trans, b_trans, dtype_in, dtype_out, accumulate;
    int64_t M, N, K, lda, ldb, ldc;
    unsigned a_bits, b_bits, c_bits, ws_bits, rowsum_bits, bias_bits, residual_bits;   // address & 15 (rowsum_bits: a_rowsum | b_rowsum)
    int64_t workspace_bytes;     // 0: none offered; < 0: a sizing query (emo_gemm_workspace_bytes) — whatever the plan asks for is there
    // epilogue features
    int act, mul_mode;           // (mul_mode: EMO_MUL_NONE without mul_aux)
    bool bias, aux_out, drop, residual, a_rowsum, b_rowsum, mask_out, ln_fused, lna, hdiv, drop_index_64;   // drop_index_64: M * N >= 2^32 with dropout
    bool has_epi() const { return bias || act || aux_out || mul_mode || drop || residual; }
};
struct GemmPlan {
    const char* error;           // non-null: emo_gemm refuses the call with this text
    int family, flags;           // emo_gemm_last_kernel(): family | flags (16: split-K through the workspace, 32: with the reduce-and-epilogue pass)
    int bk, stages, splits, col_split;      // emo_gemm_last_plan()
    int64_t kps;                 // K range of one split
    unsigned grid_x, grid_y;
    int atomic;                  // EpiParams.atomic: XCDs per split (splitk_coords), 0 = unsplit
    bool use_ws, epi_split, memset_c;       // memset_c: split-K through atomics into a C that is not accumulated onto
    bool colsum_a, colsum_b;     // the row sum asked for does not run in-kernel: a separate emo_colsum launch
    bool safe, ring;             // 128 x 128 bf16 kernels: scalar transposing reads; LDS-DMA ring (else register-staged)
    int f32_tile;                // fp32: 64 / 128
    int astat_instance, tiles_per_block;    // A-stationary: AF_* flags of the instance, column tiles per block
    int tn_full, tn_extra;       // 256 x 256 wgrad: whole splits per XCD, splits in the block slots left over
    bool tn_rs_ws;               // ... its bias-gradient partials go through the workspace (else atomics)
    int nt_store, a_nt, nt_mask, sched;     // per-launch policy bits (sched: EMO_P256_SCHED)
    int64_t ws_floats, rs_floats;           // workspace the plan asks for: product partials (before the split count is rounded to whole K tiles), bias partials
    int last_kernel() const { return family + flags; }
    int last_plan() const { return bk | stages << 8 | splits << 16 | col_split << 24; }
};
// ------------------------------------------------------------------------------------------------ gates
// A-stationary K = 512 kernel, the part that does not depend on the tensors (emo_gemm_astat_supported)
static inline bool gp_astat_class(int dtype_in, int dtype_out, int64_t M, int64_t N, int64_t K) {
    if (dtype_in != EMO_BF16 || (dtype_out != EMO_BF16 && dtype_out != EMO_F32) || gp_safe_tr()) return false;
    if (getenv("EMO_GEMM_NO_ASTAT") != nullptr) return false;
    // one block owns a 128-row panel and sweeps all of N: the grid is M / 128 blocks.  Below one panel per CU (the reference's batch_size 4:
    // 64 panels) the column tiles of a panel are split over blockIdx.y, every block keeping at least two column tiles (r05; until then these
    // shapes ran on the 128 x 128 tiling at 0.15 of the MFMA peak)
    return K == GP_AS_K && (M % GP_AS_BM) == 0 && M >= gp_astat_min_rows() && (N % GP_AS_BN) == 0 && N <= GP_AS_MAXN && N >= GP_AS_BN;
}
static inline bool gp_aligned_nt(const GemmCall& c) { return !((c.lda & 7) || (c.ldb & 7) || (c.ldc & 7) || c.a_bits || c.b_bits || c.c_bits); }
static inline bool gp_astat(const GemmCall& c, GemmPlan& p) {
    if (!gp_astat_class(c.dtype_in, c.dtype_out, c.M, c.N, c.K) || c.accumulate) return false;
    if ((c.hdiv || c.mask_out || c.mul_mode == EMO_MUL_BITMASK) && c.dtype_out != EMO_BF16) return false;
    if (c.act == EMO_ACT_GELU || c.mul_mode == EMO_MUL_DGELU) return false;          // (exact erf GELU: the generic tiled epilogue only)
    if (!gp_aligned_nt(c) || (uint64_t)(GP_AS_BN * c.ldb + GP_AS_K) * 2 >= 0xFFFF0000ull) return false;
    const int n_tiles_all = (int)(c.N / GP_AS_BN);
    int split = 1;
    // the smallest split that gives every CU one block — two for the long column sweeps (N >= 2048), where a lone block per CU leaves the MFMA pipe
    // without a partner wave for 32 column tiles (tools/bench_astat_split.py at 8192 / 16384 / 32768 rows; GPT-2 step at 32768 tokens, whose
    // products ran one block per CU: 19.0 -> 18.4 ms with two)
    const int64_t want_blocks = c.N >= 2048 ? 512 : 256;
    if (c.M / GP_AS_BM < want_blocks)
        for (int sp = 2; sp <= n_tiles_all / 2; ++sp)
            if (n_tiles_all % sp == 0) {
                split = sp;
                if ((c.M / GP_AS_BM) * sp >= want_blocks) break;
            }
    { const int64_t f = gp_env_pos("EMO_ASTAT_SPLIT", 0); if (f && n_tiles_all % f == 0) split = (int)f; }      // (tests / experiments)
    p.family = 2; p.bk = GP_AS_KS; p.stages = 4; p.col_split = split;
    p.grid_x = (unsigned)(c.M / GP_AS_BM); p.grid_y = (unsigned)split; p.tiles_per_block = n_tiles_all / split;
    // Non-temporal output stores only for the FFN1 forward (the mask-out instance: 537 MB + the mask, read back once by the FFN2 forward).  r02
    // streamed every output beyond the 256-MB MALL; r03 per-instance sweep inside the step (EMO_ASTAT_NT_MASK, same box, 3 alternations):
    // all three large outputs 46.40 ms/step, FFN1 only 46.15, none 46.45 (the A-stationary kernels then run 0.9 ms faster and the kernels that
    // read the outputs 0.7 ms slower).  PMC: with nt stores WRITE_SIZE is 1.31 x the algorithmic bytes.
    const bool beyond_mall = c.M * c.N * 2 >= (int64_t)256 << 20;
    p.nt_store = gp_env_int("EMO_ASTAT_NT", (beyond_mall && c.mask_out) ? 1 : 0);
    p.a_nt = gp_env_int("EMO_ASTAT_A_NT", 0);
    { const char* e = getenv("EMO_ASTAT_NT_MASK");                 // diagnostics: 1 = mask-out instance, 2 = bit-mask instance, 4 = the others (outputs >= 256 MB)
      if (e && beyond_mall) p.nt_store = (atoi(e) & (c.mask_out ? 1 : (c.mul_mode == EMO_MUL_BITMASK ? 2 : 4))) ? 1 : 0; }
    // feature flags of this launch; the sets the Performer layer uses have their own straight-line instantiation, the rest runs the generic one
    const bool gelu_aux = c.act == EMO_ACT_GELU_NEW && c.aux_out;
    const int fl = (c.act == EMO_ACT_RELU ? AF_RELU : 0) | (c.drop ? AF_DROP : 0) | (c.residual ? AF_RES : 0) | (c.mul_mode == EMO_MUL_BITMASK ? AF_BITS : 0) |
                   (c.mask_out ? AF_MASKOUT : 0) | (c.mul_mode == EMO_MUL_DGELU_NEW ? AF_DGELU : 0) | (gelu_aux ? AF_GELUAUX : 0);
    const bool other = (!gelu_aux && (c.aux_out || c.act == EMO_ACT_GELU_NEW)) || c.mul_mode == EMO_MUL_NONZERO || c.drop_index_64;
    // (relu + dropout WITHOUT the mask output — no caller in the training or decoding paths — runs the generic instance: its straight-line
    // instantiation no longer fits 256 VGPRs without an in-loop reload, which drains the ring)
    const bool own = fl == 0 || fl == AF_RELU || fl == (AF_RELU | AF_DROP | AF_MASKOUT) || fl == AF_RES || fl == (AF_DROP | AF_RES) || fl == AF_BITS ||
                     fl == AF_DGELU || fl == AF_GELUAUX;
    p.astat_instance = c.hdiv ? AF_HDIV : ((c.dtype_out == EMO_F32 || other || !own) ? AF_GENERIC : fl);      // (emo_gemm admits hdiv only with a plain epilogue)
    return true;
}
// register epilogue of the 256 x 256 / 128 x 512 tile NT kernels: bias, dropout, residual
static inline bool gp_tile_nt_epilogue(const GemmCall& c) {
    return !c.accumulate && !c.mask_out && !c.aux_out && c.mul_mode == EMO_MUL_NONE && c.act == EMO_ACT_NONE && gp_aligned_nt(c);
}
// NT bf16 product on 256 x 256 tiles, one wave per SIMD.  Default: long reductions (K >= 1024) with at least one tile per CU; EMO_GEMM_W128=0 switches
// it off, =1 admits every eligible shape (tests).
static inline bool gp_w128_nt(const GemmCall& c, GemmPlan& p) {
    const int mode = gp_env_int("EMO_GEMM_W128", -1);
    if (mode == 0) return false;
    if ((c.M % GP_W_BM) || (c.N % GP_W_BN) || (c.K % GP_W_BK) || c.K < 4 * GP_W_BK || c.dtype_out != EMO_BF16) return false;
    if (mode < 0 && (c.K < 1024 || (c.M / GP_W_BM) * (c.N / GP_W_BN) < 256)) return false;
    if (!gp_tile_nt_epilogue(c) || (uint64_t)(256 * (c.lda > c.ldb ? c.lda : c.ldb) + 64) * 2 >= 0xFFFF0000ull) return false;
    p.family = 4; p.bk = GP_W_BK; p.stages = GP_W_STAGES;
    p.grid_x = (unsigned)(gp_cdiv(c.M / GP_W_BM, 8) * 8 * (c.N / GP_W_BN));
    p.nt_store = gp_env_int("EMO_W128_NT_STORE", 0);
    p.a_nt = gp_env_int("EMO_W128_A_NT", 1);                   // default on (r03: -0.4 .. -0.55 ms/step; the wgrad kernel loses with it)
    return true;
}
// K-splits of the TN (wgrad) product on 256 x 256 tiles (at most one block per CU, see the kernel's block mapping); 0 = shape not taken.
static inline int64_t gp_w128_tn_splits(int64_t M, int64_t N, int64_t K, int& full, int& extra) {
    full = extra = 0;
    if (gp_env_int("EMO_GEMM_W128", 1) == 0) return 0;
    const int tn = gp_env_int("EMO_GEMM_W128_TN", 1);
    if (tn == 0) return 0;
    if ((M % GP_W_BM) || (N % GP_W_BN) || (K % GP_W_BK)) return 0;
    const int64_t ntile = (M / GP_W_BM) * (N / GP_W_BN), nkt = K / GP_W_BK;
    if (ntile > 32) return 0;
    int64_t f = 32 / ntile;
    if (f > 8) f = 8;                                          // at most 64 splits
    int64_t x = f < 8 ? (8 * (32 - f * ntile)) / ntile : 0;
    if (tn == 2) x = 0;                                        // (diagnostics: whole splits per XCD only)
    // K-tiles per split (r04: 8 let batch-size-4 steps — 512 tokens per split — onto this tile, where prologue + epilogue dominate: 8.89 vs 8.39 ms per step)
    const int64_t min_kt = gp_env_pos("EMO_W128_TN_MINKT", 16);
    while (nkt / (8 * f + x) < min_kt) {
        if (x) x = 0;
        else if (f > 1) --f;
        else return 0;
    }
    // too few blocks for the chip: the 128 x 128 kernel's finer tiles win (r04: 160 -> 96 lets the batch-size-4 FFN / QKV weight gradients on: 8.30 -> 7.97 ms per step)
    if (ntile * (8 * f + x) < gp_env_pos("EMO_W128_TN_MINBLK", 96)) return 0;
    full = (int)f;
    extra = (int)x;
    return 8 * f + x;
}
// dW[M,N] (+)= A[K,M]^T B[K,N], fp32 out, contiguous C, split-K through the caller's workspace (>= splits * M * N floats; behind them, when there is room,
// the bias-gradient partials: one vector per (split, tile of the other dimension))
static inline bool gp_w128_tn(const GemmCall& c, bool a_rs, bool b_rs, GemmPlan& p) {
    int full, extra;
    const int64_t splits = gp_w128_tn_splits(c.M, c.N, c.K, full, extra);
    const bool sizing = c.workspace_bytes < 0;
    if (!splits || c.ldc != c.N || c.workspace_bytes == 0 || c.ws_bits || (!sizing && c.workspace_bytes < splits * c.M * c.N * (int64_t)sizeof(float))) return false;
    if ((c.lda & 7) || (c.ldb & 7) || c.a_bits || c.b_bits || c.c_bits) return false;
    if ((uint64_t)(64 * (c.lda > c.ldb ? c.lda : c.ldb) + 256) * 2 >= 0xFFFF0000ull) return false;
    const int64_t ra = (c.N / GP_W_BN) * c.M, rb = (c.M / GP_W_BM) * c.N;
    p.family = 3; p.bk = GP_W_BK; p.stages = GP_W_STAGES; p.splits = (int)splits;
    p.kps = gp_cdiv(c.K / GP_W_BK, splits) * GP_W_BK;
    p.grid_x = 256;                                            // 32 block slots per XCD
    p.tn_full = full; p.tn_extra = extra; p.nt_mask = gp_env_int("EMO_W128_TN_NT", 0);
    p.ws_floats = splits * c.M * c.N;
    p.rs_floats = splits * (ra > rb ? ra : rb);
    p.tn_rs_ws = (a_rs || b_rs) && (sizing || c.workspace_bytes >= (p.ws_floats + p.rs_floats) * (int64_t)sizeof(float)) && !c.rowsum_bits;
    p.use_ws = true;                                           // (always: the kernel has no other way out; not reported as + 16)
    return true;
}
#ifdef EMO_EXPERIMENTAL
// Opt-in persistent tile walks (r05).  128 x 512 tile: EMO_GEMM_Q512 = 1 every eligible shape, 2 long reductions only; EMO_Q512_PERSIST=1: one workgroup
// per CU walking its tiles instead of one tile per workgroup.  256 x 256 tile: EMO_GEMM_P256 likewise (tests, tools/bench_p256.py); unset / 0 = off
// (behind the tile-per-block kernel inside the training step, profiles/r05_gemm_isa_diff.txt).
static inline bool gp_persistent(const GemmCall& c, GemmPlan& p) {
    for (int fam = 9; fam >= 8; --fam) {
        const int64_t bm = fam == 9 ? 128 : 256, bn = fam == 9 ? 512 : 256;
        const int mode = gp_env_int(fam == 9 ? "EMO_GEMM_Q512" : "EMO_GEMM_P256", 0);
        if (mode <= 0) continue;
        if ((c.M % bm) || (c.N % bn) || (c.K % 32) || c.K < 64 || c.dtype_out != EMO_BF16) continue;
        if (mode == 2 && (c.K < 1024 || (c.M / bm) * (c.N / bn) < 256)) continue;
        if (!gp_tile_nt_epilogue(c) || (c.residual && c.residual_bits) || (c.bias && c.bias_bits)) continue;
        if ((uint64_t)(bn * (c.lda > c.ldb ? c.lda : c.ldb) + 64) * 2 >= 0x7FFF0000ull) continue;
        int64_t nslot = gp_cdiv((c.M / bm) * (c.N / bn), 8);
        if ((fam == 8 || gp_env_int("EMO_Q512_PERSIST", 0)) && nslot > 32) nslot = 32;       // one workgroup per CU
        p.family = fam;
        p.grid_x = (unsigned)(8 * nslot);
        if (fam == 8) { p.nt_store = gp_env_int("EMO_P256_SKEW", 0); p.sched = gp_env_int("EMO_P256_SCHED", 0); }
        return true;
    }
    return false;
}
#endif
// fp32 products: tile edge of the kernel that serves the shape.  EMO_GEMM_F32_TILE=64 keeps every shape on the 64 x 64 kernel (A/B, tests).
static inline int gp_f32_tile(int64_t M, int64_t N) { return (gp_env_int("EMO_GEMM_F32_TILE", 0) != 64 && M >= 128 && N >= 128) ? 128 : 64; }
// K-splits of a bf16-output product with an epilogue (0 / 1 = none): a tile grid of at most 128 blocks and a long reduction
static inline int64_t gp_epi_splits(int64_t M, int64_t N, int64_t K) {
    if (gp_env_int("EMO_GEMM_EPI_SPLIT", 1) == 0 || (N & 7) || (K % (4 * GP_RING_BK)) != 0) return 1;
    // measured r04 (same-box A/B script of that round, rocprofv3 per kernel; profiles/r04_ab_epi_split*): stage 1's K = 2048 dgrads on 64 tiles 48 -> 22 + 6 us with 4 splits; at 256 tiles
    // (batch-size-4 stage-2 dgrads) 2 splits only tie (52 -> 45 + 15 us: the 32 MB of fp32 partials cost what the second resident block gains)
    if (gp_cdiv(M, GP_BM) * gp_cdiv(N, GP_BN) > 128) return 1;
    // (K = 512 products on <= 64 tiles, 4 splits: 18.6 -> 13.4 + 5 us per launch, the step's kernel time unchanged at 89.9 vs 89.8 ms: not split)
    return K >= 1024 ? 4 : 1;
}
// number of K-splits for a plain fp32-output GEMM (wgrad).  max_ws_splits > 0: partials go to a caller workspace (plain stores +
// splitk_reduce_kernel); 0: fp32 atomics into C.
static inline int64_t gp_splits(const GemmCall& c, bool big, int64_t BMt, int64_t BNt, int64_t BKt, int64_t max_ws_splits) {
    const int64_t tiles_m = gp_cdiv(c.M, BMt), tiles_n = gp_cdiv(c.N, BNt);
    int64_t splits = 1;
    if (c.dtype_out == EMO_F32 && !c.has_epi() && tiles_m * tiles_n < 256 && c.K >= 8 * BKt) {
        const int64_t max_splits = c.K / (4 * BKt);
        if (big) {
            // Cost model fitted to the r01 sweep (tools/bench_wgrad_splits.py of that round — git history —, M = 8k/32k/131k tokens): a 128^2 x 64 K-step takes ~1.1 us
            // with one block per CU and ~1.4 us with two; blocks run in rounds of 512 (2 per CU); every split pays ~0.18 us per output
            // tile for its fp32 atomics (device-scope atomics from 8 XCDs resolve beyond the L2s: ~0.3 TB/s), or ~0.03 us per tile for
            // plain stores + its share of the reduce pass when a workspace is available.
            static const int cand[] = {1, 2, 4, 8, 16, 24, 32};
            const double tiles = (double)(tiles_m * tiles_n), ksteps = (double)gp_cdiv(c.K, BKt);
            const double per_split = max_ws_splits > 0 ? 0.03 : 0.18;
            double best = 1e30;
            for (int s : cand) {
                if (s > 1 && (s > max_splits || (max_ws_splits > 0 && s > max_ws_splits))) break;
                const double blocks = tiles * s, rounds = (double)gp_cdiv((int64_t)blocks, 512);
                const double t = rounds * (double)gp_cdiv((int64_t)ksteps, s) * (blocks > 256 ? 1.4 : 1.1) + s * tiles * per_split;
                if (t < best) { best = t; splits = s; }
            }
        } else {
            splits = gp_cdiv(512, tiles_m * tiles_n);
            if (splits > max_splits) splits = max_splits;
            if (splits >= 4) {                       // one K-split per XCD round (splitk_coords): keep the 8 XCDs evenly loaded
                const int64_t r8 = gp_cdiv(splits, 8) * 8;
                splits = r8 <= max_splits ? r8 : ((splits / 8) * 8 > 0 ? (splits / 8) * 8 : splits);
            }
            if (max_ws_splits > 0 && splits > max_ws_splits) splits = max_ws_splits;
        }
        if (splits < 1) splits = 1;
        { const int64_t fs = gp_env_pos("EMO_GEMM_SPLITS", 0); if (fs > 0) splits = fs <= max_splits ? fs : max_splits; }   // tuning sweeps
    }
    return splits;
}
// the 128 x 128 bf16 tiles (LDS-DMA ring / register-staged) and the fp32 kernels: split-K, grid, ring geometry
static inline void gp_tiled(const GemmCall& c, bool a_rs, bool b_rs, int variant, GemmPlan& p) {
    const bool big = c.dtype_in == EMO_BF16, sizing = c.workspace_bytes < 0;
    p.f32_tile = big ? 0 : gp_f32_tile(c.M, c.N);
    const int64_t BMt = big ? GP_BM : p.f32_tile, BNt = big ? GP_BN : p.f32_tile;
    const int64_t BKt = big ? (variant >= 2 ? GP_RING_BK : GP_BK) : 16;
    const int64_t tiles_m = gp_cdiv(c.M, BMt), tiles_n = gp_cdiv(c.N, BNt);
    // split-K: only for plain fp32 outputs (wgrad) when the tile grid cannot fill the chip
    // (a sizing query is answered as if the workspace could be used: its size has never depended on M * N % 4 or EMO_GEMM_SPLIT_ATOMIC)
    const bool ws_ok = sizing || (c.workspace_bytes != 0 && c.ldc == c.N && ((c.M * c.N) & 3) == 0 && !c.ws_bits && getenv("EMO_GEMM_SPLIT_ATOMIC") == nullptr);
    const int64_t max_ws_splits = !ws_ok ? 0 : (sizing ? GP_MAX_SPLITS : c.workspace_bytes / (c.M * c.N * (int64_t)sizeof(float)));
    int64_t splits = gp_splits(c, big, BMt, BNt, BKt, max_ws_splits >= 2 ? max_ws_splits : 0);
    if (c.ldc != c.N) splits = 1;                            // split-K partials need a contiguous C: a strided output view runs unsplit
    // bf16 outputs (with or without an epilogue) on a small tile grid: split-K through the workspace + the reduce-and-epilogue pass
    if (big && c.dtype_out == EMO_BF16 && !c.accumulate && ws_ok && variant >= 2 && !p.safe && (!c.a_trans || variant >= 3) && !a_rs && !b_rs) {
        const int64_t es = gp_epi_splits(c.M, c.N, c.K);
        if (es > 1 && max_ws_splits >= es) { splits = es; p.epi_split = true; }
    }
    if (splits > 1 && (sizing || max_ws_splits >= splits)) p.ws_floats = splits * c.M * c.N;
    p.kps = gp_cdiv(gp_cdiv(c.K, splits), BKt) * BKt;
    splits = gp_cdiv(c.K, p.kps);
    p.use_ws = splits > 1 && max_ws_splits >= splits;
    p.grid_x = (unsigned)(gp_cdiv(tiles_m, 8) * 8 * tiles_n);
    if (splits > 1) {   // see splitk_coords()
        p.atomic = (splits == 2 || splits == 4) ? (int)(8 / splits) : 1;
        p.memset_c = !p.use_ws && !c.accumulate;
        p.grid_x = p.atomic > 1 ? (unsigned)(8 * gp_cdiv(tiles_m * tiles_n, p.atomic)) : (unsigned)(tiles_m * tiles_n * (gp_cdiv(splits, 8) * 8));
    }
    p.flags = p.use_ws ? (p.epi_split ? 32 : 16) : 0; p.splits = splits > 1 ? (int)splits : 0;
    if (!big) { p.family = 7; p.bk = 16; return; }
    if ((c.lda & 7) || (c.ldb & 7)) { p.error = "emo_gemm(bf16): lda/ldb must be multiples of 8 (16-B rows)"; return; }
    if (c.a_bits || c.b_bits) { p.error = "emo_gemm(bf16): A/B must be 16-B aligned"; return; }
    const int64_t rowsA = c.a_trans ? GP_RING_BK : c.M, rowsB = c.b_trans ? GP_RING_BK : c.N;
    const int64_t spanA = (rowsA * c.lda + (c.a_trans ? c.M : 0)) * 2, spanB = (rowsB * c.ldb + (c.b_trans ? c.N : 0)) * 2;
    p.ring = !p.safe && variant >= 2 && (!c.a_trans || variant >= 3) && (c.K % GP_RING_BK) == 0 && (p.kps % GP_RING_BK) == 0 && c.M >= 8 && c.N >= 8 &&
             spanA < (int64_t)0xFFFF0000 && spanB < (int64_t)0xFFFF0000;
    if (!p.ring) { p.family = 6; p.bk = GP_BK; return; }     // register-staged v1 (same 128^2 grid; any K, predicated edges)
    p.family = 5;
    // measured r01 (tools/bench_gemm.py of that round — git history — MI355X): the per-tile fixed cost (prologue latency + epilogue, ~4-5 us) is what
    // limits the K=512 GEMMs, so OCCUPANCY wins over prefetch depth: a 3-stage ring of 32-deep tiles (48 KB LDS, 3 blocks
    // per CU) beats the 4-stage ring (64 KB, 2 blocks) by 13-16 % (qkv 575 vs 509, ffn1 659 vs 568 TFLOP/s); for the
    // long reduction (K=2048) the double buffer of full 128-B lines is best (842 vs 796); for MN-contiguous B (dgrad)
    // the 2-stage ring of 32-deep tiles (32 KB, 4 blocks per CU) is best (in-step A/B of the other geometries: DESIGN.md §4.1).
    const bool can64 = (p.kps % 64) == 0 && (c.K % 64) == 0;
    // Small grids (at most two tiles per CU: the reference YAML's batch size 4, stage 1): occupancy has nothing to offer, a block is alone on
    // its CU and every K step exposed an L2 / HBM round trip -> the 4-stage ring of 32-deep tiles (three tiles in flight inside the block)
    // (r03, same box: batch-4 step 8.85 -> 8.79 ms, stage 1 7.64 -> 7.47 ms; a 64-deep double buffer instead was erratic: 8.5 / 9.2 ms)
    if (p.grid_x <= 512 && gp_small_grid_ring() && c.K >= 128) {
        // 64-deep tiles in the same 4-stage ring = twice the bytes in flight per block (128 KB of LDS, one block per CU): what bounds these products is
        // the bytes one block keeps in flight (r04, same box, two pairs: stage 1 262 / 266 -> 284 / 283 k tokens/s, batch-size-4 steps unchanged)
        p.stages = 4;
        p.bk = (gp_small_grid_bk64() && can64 && p.kps >= 512) ? 64 : 32;
    } else if (!c.b_trans && c.K > 1024 && can64) { p.bk = 64; p.stages = 2; }
    else { p.bk = 32; p.stages = c.b_trans ? 2 : 3; }
}
// ------------------------------------------------------------------------------------------------ the planner
// The call has passed emo_gemm's argument checks (dtypes, the pointer sets of lna_* / hdiv / rln_*, a_rowsum / b_rowsum with their layouts).
static inline GemmPlan gemm_plan(const GemmCall& c) {
    GemmPlan p = {};
    const bool big = c.dtype_in == EMO_BF16, nt = !c.a_trans && !c.b_trans;
    const int variant = big ? gp_variant(c.a_trans, c.K) : 0;
    p.safe = gp_safe_tr();
    // bias gradient: in-kernel on the register-staged wgrad instances and the 256 x 256 wgrad kernel, else the plain column-sum launch over the operand
    const bool rs_in_kernel = big && c.dtype_out == EMO_F32 && c.b_trans && variant < 3 && !p.safe;
    p.colsum_a = c.a_rowsum && !rs_in_kernel;
    p.colsum_b = c.b_rowsum && !rs_in_kernel;
    const bool a_rs = c.a_rowsum && rs_in_kernel, b_rs = c.b_rowsum && rs_in_kernel;
    if (big && c.M <= 32 && nt && (c.K % 32) == 0 && (c.lda & 7) == 0 && (c.ldb & 7) == 0 && !c.a_bits && !c.b_bits && !c.accumulate) {
        p.family = 1;                                        // skinny (decode step); plan fields: chunk width, waves
        p.stages = c.K >= 2048 ? 16 : (c.K >= 1024 ? 8 : 4);   // 16 waves x two 64-wide chunks at K = 2048
        p.bk = p.stages >= 16 ? 64 : 128;
        p.grid_x = (unsigned)gp_cdiv(c.N, 16);
        return p;
    }
#ifdef EMO_EXPERIMENTAL
    if (big && nt && !c.ln_fused && !p.safe && !c.lna && !c.hdiv && gp_persistent(c, p)) return p;
#endif
    if (big && nt && !c.ln_fused && gp_astat(c, p)) return p;                                     // K = 512, A stationary in registers
    if (big && c.a_trans && c.b_trans && c.dtype_out == EMO_F32 && !c.has_epi() && !c.ln_fused && !p.safe && gp_w128_tn(c, a_rs, b_rs, p)) return p;
    if (c.lna) p.error = "emo_gemm: lna_* (LayerNorm of the A operand) exists only on the A-stationary kernel: bf16, NT, K = 512, M % 128 == 0, M >= 4096, N % 64 == 0, N <= 2048";
    else if (c.hdiv) p.error = "emo_gemm: hdiv exists only on the A-stationary kernel and this call was refused by it (alignment / strides / EMO_GEMM_NO_ASTAT)";
    else if (big && nt && !c.ln_fused && gp_w128_nt(c, p)) return p;                              // long-K NT products on 256 x 256 tiles
    else if (c.mask_out || c.mul_mode == EMO_MUL_BITMASK) p.error = "emo_gemm: mask_out / EMO_MUL_BITMASK need bf16 in/out, NT, K = 512, M % 128 == 0, M >= 4096, N % 64 == 0, N <= 2048";
    else if (c.ln_fused) p.error = "emo_gemm: the LayerNorm-folded epilogue (ln_c1 / rln_x) exists only on the skinny path (bf16, M <= 32, NT, K % 32 == 0)";
    else gp_tiled(c, a_rs, b_rs, variant, p);
    return p;
}
