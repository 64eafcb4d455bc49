/* idf.h -- C ABI of libidf_gfx950.so: hand-written HIP/CDNA4 kernels for the InstanceDiffusion sampling path.
 *
 * The reference (frank-xwang/InstanceDiffusion) is pure Python and has NO FFI: every arithmetic op on its hot
 * path is a PyTorch ATen call.  Each entry point below REPLACES one family of those ATen call sites; the
 * reference file:line it replaces is cited per function (paths relative to the reference repo root).
 * A reference maintainer binds these with ctypes.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM) unless named h_*; no function allocates, frees or synchronises;
 *   - every launcher enqueues on `stream` (a hipStream_t passed as void*) and is hipGraph-capturable;
 *   - return: 0 ok; <0 invalid argument (IDF_E_*); >0 a hipError_t from the launch;
 *   - activations are NHWC / token-major row-major matrices in 16-bit storage (dtype enum below), fp32 accumulate;
 *   - "ld*" are leading dimensions in ELEMENTS; 16-byte alignment of every row start is required.
 */
#ifndef IDF_H_
#define IDF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDF_ABI_VERSION 5

enum { IDF_BF16 = 0, IDF_F16 = 1 };                 /* 16-bit storage / MFMA input type */
enum { IDF_E_ARG = -1, IDF_E_ALIGN = -2, IDF_E_UNSUPPORTED = -3 };

/* epilogue flags for idf_gemm / idf_conv3x3 (bitmask) */
enum {
  IDF_EPI_BIAS     = 1,    /* + bias[n]                       (f32 [N])                                   */
  IDF_EPI_ROWBIAS  = 2,    /* + rowbias[m / rows_per_batch][n] (16-bit [*, ld_rowbias])  -- time-embedding */
  IDF_EPI_RES      = 4,    /* + res[m][n]                     (16-bit, ldr)                                */
  IDF_EPI_GATE     = 8,    /* out = res + gate[0] * (acc + bias)   (gate: f32 device scalar); needs RES    */
  IDF_EPI_SILU     = 16,   /* out = silu(acc + bias)                                                       */
  IDF_EPI_GELU     = 32,   /* out = gelu_erf(acc + bias)                                                   */
  IDF_EPI_GEGLU    = 64,   /* weight rows interleaved [32 value | 32 gate] per 64; out[m][j] = v * gelu(g) */
  IDF_EPI_OUT_F32  = 128,  /* store fp32 instead of 16-bit                                                 */
  IDF_EPI_OUT_NCHW = 256,  /* conv only: store fp32 NCHW [B, n_valid, Ho, Wo] (final out conv)             */
  /* LayerNorm of an operand folded into the GEMM (attention.py:294-295,320-322: x -> LN(x) -> Linear):
   *   LN(x) W^T = rstd_m * (x (gamma*W)^T - mu_m * c) + d,   c[n] = sum_k (gamma*W)[n][k],  d[n] = sum_k beta[k] W[n][k] (+ bias[n])
   * so the raw 16-bit x goes through the MFMAs against the gamma-folded weight and the epilogue applies the per-row
   * statistics -- the normalised activation is never written to or read from HBM.  ln_stats = [rows][2] f32 (mu, rstd) of
   * the NORMALISED operand: LN_ROW = A's rows (index m); LN_COL = W's rows (index n: the transposed-V projection, whose
   * "weight" operand is the token matrix).  ln_c is indexed the other way (n for LN_ROW, m for LN_COL); d travels as
   * `bias` (LN_ROW, needs BIAS) / `rowvec` (LN_COL).  With GEGLU both accumulators of a pair are corrected before the GELU. */
  IDF_EPI_LN_ROW   = 512,
  IDF_EPI_LN_COL   = 1024,
  /* modifier of IDF_EPI_GEGLU: the weight rows are interleaved [16 value | 16 gate] per 32 instead of [32 | 32] per 64.  Value
   * and gate of an output then sit in ONE 32-wide MFMA fragment (registers q and q + 2 of a lane), so the wave tile no longer
   * needs an even number of fragments and the GEGLU GEMMs run on the 320-wide persistent tiles (N % 320 == 0). */
  IDF_EPI_GEGLU_P32 = 2048,
  /* idf_gemm only: out = y * sigmoid(1.702 y), y = acc + bias -- the "quick_gelu" of the CLIP text transformer's MLP
   * (ldm/modules/encoders/modules.py:144-172 -> CLIPTextModel).  Composes with BIAS and LN_ROW (and RES / OUT_F32 like the other
   * activations); with SILU, GELU or GEGLU it is IDF_E_ARG.  Every idf_gemm kernel family implements it (the persistent kernel, the
   * small-tile and latency kernels and the split-K reducer); the fused q | k | v form (vt_out) and the convs reject it. */
  IDF_EPI_QUICKGELU = 4096
};

int idf_abi_version(void);
const char* idf_build_info(void);

/* Kernel-selection knobs (process-global, for A/B measurement and for tests that must hit one specific kernel;
 * results are identical up to fp32 summation order).  Returns the previous value, or IDF_E_ARG for an unknown knob / value.
 *   IDF_TUNE_GEMM_BIG: 0 = never use the persistent 256 x {320,256,128}-tile GEMM/conv kernel, 1 = automatic
 *   (shape + tile-quantisation rule), 2 = whenever the shape qualifies, 3 = automatic + HYBRID TAIL SPLIT: a tile count just
 *   above a whole number of 256-CU rounds (the 18-row forwards of a sharded / small batch) runs its leading full rounds as whole
 *   tiles and cuts only the tail rows into K-slices instead of falling back to the 128x128 kernels (3x3 conv 536 -> 709 TF at
 *   18 rows).  Opt-in, because the tail rows are then summed in another order than the rows of the whole tiles: identical
 *   rows of one launch are no longer bitwise equal, the property modes 0..2 keep.  Initial value: env IDF_GEMM_BIG or the default (1).
 *   IDF_TUNE_ATTN2: 0 = attention always on the 32-queries-per-wave kernel; 1 = when the shape qualifies
 *   (d in {24,40,56}, n0 % 8 == n1 % 8 == 0, no mask) the 64-queries-per-wave LDS-DMA kernel (attention4.hip: max-free
 *   softmax with the reference value folded into the K.Q^T MFMA, K fragments read one tile ahead, XCD-aware 1-D grid) as two
 *   4-wave workgroups per CU (256 queries each); 2 = the same kernel as one 8-wave workgroup per 512 queries; 3 = mode 1
 *   with the plain block order (A/B of the XCD mapping); 4 / 5 (round 6, d = 40 only; other head dims run as mode 1) = the
 *   asm-scheduled stream of attention4w.hip -- every MFMA, v_exp, v_cvt_pk and LDS read of the tile loop in program order,
 *   accumulators / Q / V^T fragments in asm-owned AGPRs, no per-tile overflow guard (one finiteness check per block, exact
 *   rerun otherwise) -- with 128 queries per wave and one wave per SIMD (4) or 64 queries per wave and two 4-wave workgroups
 *   per CU (5; the default: +6..8 % over mode 1 in isolation, -1.2 % on a 128-row forward).  Results of modes 1, 4, 5 are
 *   bit-identical unless a re-base / rerun path is taken.  6 = mode 4 as a persistent workgroup that prefetches the next query
 *   block: measured 1-2 % slower, only in experiment builds of attention4w.hip (else served as mode 1).
 *   Initial value: env IDF_ATTN2 or the default (5).
 *   IDF_TUNE_GEMM_RING (round 4): the launches the persistent kernel declines (small batches: every GEMM / conv of a 2-row
 *   forward) go to the LATENCY kernel -- the 128 x {128,64} tiles of the default small-tile kernels with a 4-5-stage LDS-DMA
 *   ring that has its K-tiles in flight from the first instruction instead of one at a time -- when their tile grid has at most
 *   `value` tiles; 0 = never.  Same tiles, same K order: the result bits do not depend on it unless the split-K choice differs.
 *   Initial value: env IDF_GEMM_RING or the library default.
 *   IDF_TUNE_BIG_MIN_EFF (round 4): occupancy bar of IDF_TUNE_GEMM_BIG's automatic rule in per cent (1..100): the persistent
 *   kernel takes a launch whose tile grid fills at least this share of the workgroup slots of its last round.  Initial value:
 *   env IDF_BIG_MIN_EFF or the library default.
 * (ABI 2 also exposed the kernel variants that were measured slower -- GEMM geometries 1..6, attention modes 1..14; they
 * left the library in ABI 3 and live under profiles/archive_rejected_kernels/ with their measurements in profiles/r02_*.)
 *   IDF_TUNE_ATTN8 (round 5, ABI 5): the d = 80 / d = 160 self and gated self-attention (n0 % 8 == n1 % 8 == 0, no mask) on the
 *   LDS-DMA kernel of attention8.hip (32 queries per wave, K / V^T rings, deferred-rescale running max, XCD-aware 1-D grid):
 *   0 = off (the register-staged 32-query kernel), 1 = on (d = 80: two 4-wave workgroups per CU; d = 160: one 8-wave workgroup
 *   per 256 queries, 4-wave workgroups below), 2 = 8-wave workgroups throughout, 3 = mode 1 with the plain block order,
 *   4 = d = 160 on 4-wave workgroups, 5 / 6 = d = 80 software-pipelined on 4- / 8-wave workgroups.
 *   Initial value: env IDF_ATTN8 or the default (1).
 *   IDF_TUNE_MLP (round 6; a knob id, no new entry point): idf_mlp_geglu on 0 = mlp320_kernel (8 waves, two per SIMD),
 *     1 = mlp320w_kernel (4 waves, one generated instruction stream per SIMD; default).  Same results bit for bit.  Env IDF_MLP_MODE.
 *   IDF_TUNE_QKV_ROW (round 6): the fused q | k | v projection of the C = 320 level (K = 320, N = 960, vt_col0 = 640, M % 256 == 0) and
 *     of the C = 640 level (K = 640, N = 1920, vt_col0 = 1280, M % 128 == 0), statistics handed in, from two tiles per CU, on
 *     qkv320w_kernel / qkv640w_kernel (activation rows resident in registers): 0 = never, 1 = when the shape qualifies (default).
 *     Env IDF_QKV_ROW.  Same per-element error against fp64 as the persistent kernel; the two round 0.1 % of the outputs apart (one
 *     16-bit ulp) at |mean| / std < 1 of the rows, a share that grows in proportion to that ratio (up to 9 % at 100): the mean term
 *     is folded as a k-step of 16-bit hi + lo products, not as an fp32 fma behind the sum (csrc/qkv_fused.hip).
 *   IDF_TUNE_GEGLU_ROW (round 6): the GEGLU projection of the C = 640 level (K = 640, N = 5120, epilogue BIAS | GEGLU | GEGLU_P32 |
 *     LN_ROW with the statistics handed in, M % 128 == 0, from two tiles per CU) on geglu640w_kernel: 0 = never, 1 = when the shape
 *     qualifies (default).  Env IDF_GEGLU_ROW.  Same per-element error against fp64 as the persistent kernel; the two round up to
 *     0.2 % of the outputs apart at |mean| / std < 1 of the rows, up to 12 % (fp16; 1.5 % bf16) at a ratio of 100, one ulp at most.
 *   IDF_TUNE_PROJ_ROW (knob 9; new enum values within ABI 5; id 8 stays unassigned -- it is the id the C-ABI test probes as
 *     the unknown knob, idf_set_tuning(8, ..) == IDF_E_ARG): the N = K = 320 projections of the C = 320 level (batch 1, no vt_out,
 *     M % 32 == 0, M >= 512 x the CU count -- two 256-row tiles per CU, the rule of IDF_TUNE_QKV_ROW; epilogue BIAS, BIAS | RES, BIAS | RES | GATE, or BIAS | LN_ROW with the statistics
 *     handed in; each with or without out_stats) on proj320s_kernel (proj320_stream.hip: the weights resident in registers, the
 *     rows streaming through LDS; out_stats come out final, no finalize pass): 0 = never (the launches of the library without this
 *     kernel, bit for bit), 1 = when the shape qualifies (default).  Env IDF_PROJ_ROW.
 *   IDF_TUNE_GEMM_BIG = 0 bypasses every row / streaming kernel above as well (QKV_ROW, GEGLU_ROW, PROJ_ROW): mode 0 is the
 *     independent small-tile reference.
 */
enum { IDF_TUNE_GEMM_BIG = 0, IDF_TUNE_ATTN2 = 1, IDF_TUNE_GEMM_RING = 2, IDF_TUNE_BIG_MIN_EFF = 3, IDF_TUNE_ATTN8 = 4, IDF_TUNE_MLP = 5,
       IDF_TUNE_QKV_ROW = 6, IDF_TUNE_GEGLU_ROW = 7, IDF_TUNE_PROJ_ROW = 9 /* 8 unassigned */ };
int idf_set_tuning(int knob, int value);
/* Process-global launch counters (tests assert which kernel served a call).  Unknown stat: -1. */
enum { IDF_STAT_GEMM_BIG_LAUNCHES = 0, IDF_STAT_ATTN2_LAUNCHES = 1, IDF_STAT_GEMM_RING_LAUNCHES = 2, IDF_STAT_ATTN8_LAUNCHES = 3,
       IDF_STAT_GN_EPI_LAUNCHES = 4 /* idf_conv3x3 calls whose gn_partial came out of the conv epilogue, not the statistics pass */,
       IDF_STAT_QKV_ROW_LAUNCHES = 6 /* fused q | k | v projections served by qkv320w_kernel (also counted in stat 0) */,
       IDF_STAT_GEGLU_ROW_LAUNCHES = 7 /* GEGLU projections served by geglu640w_kernel (also counted in stat 0) */,
       IDF_STAT_PROJ_ROW_LAUNCHES = 8 /* N = K = 320 projections served by proj320s_kernel (also counted in stat 0) */,
       IDF_STAT_PROJ_ROW_MIN_M = 9 /* not a counter: the least M proj320s_kernel takes on the current device under the current knobs
                                      (0 = IDF_TUNE_PROJ_ROW or IDF_TUNE_GEMM_BIG is 0), so a caller can plan who produces ln_stats */,
       IDF_STAT_ATTN_RES_LAUNCHES = 10 /* idf_attention calls served by the resident-key form of the 32-query kernel (<= 2 key tiles staged
                                          once per workgroup, which walks several query blocks); a new enum value within ABI 5, as knob 9 was;
                                          stat id 5 stays unassigned */,
       IDF_STAT_CLIP_PREPROC_LAUNCHES = 12 /* idf_clip_crop_resize launches; a new enum value within ABI 5; id 11 stays unassigned -- it is
                                              the id the C-ABI tests probe as the first unknown counter, idf_get_stat(11) == -1 */,
       IDF_STAT_SKIP_FOLD_LAUNCHES = 13 /* idf_conv3x3_skip calls that ran (also counted in stat 0); a new enum value within ABI 5 */ };
long long idf_get_stat(int stat);

/* ---- GEMM: out[M,N] = epi( A[M,K] . W[N,K]^T ) ----------------------------------------------------------
 * Replaces F.linear / 1x1 nn.Conv2d call sites: attention.py:39,59,106-110,168-172,289,349-364;
 * openaimodel.py:199-205,222,360-364; text_grounding_net.py:73-81,293-298.
 * Batched over `batch` with element strides (0 = shared).  K % 64 == 0.  With GEGLU, N counts packed W rows
 * (= 2x output columns).                                                                                    */
typedef struct {
  const void* A; const void* W; void* out;
  const float* bias; const void* rowbias; const void* res; const float* gate;
  int M, N, K;
  int lda, ldw, ldo, ldr, ld_rowbias;
  int rows_per_batch;                 /* ROWBIAS: rowbias row = m / rows_per_batch                          */
  int batch; long long strideA, strideW, strideO, strideR;
  int epi; int dtype;
  void* ws; long long ws_bytes;       /* optional fp32 split-K workspace (NULL = never split); used when the tile   */
                                      /* grid cannot fill 256 CUs: slices write partial slabs, a reducer applies epi */
  /* LayerNorm folded into the GEMM (IDF_EPI_LN_ROW / IDF_EPI_LN_COL, see above) */
  const float* ln_stats; long long stride_ln_stats;   /* [rows][2] (mu, rstd) of the normalised operand; batch stride in floats */
  const float* ln_c;                  /* f32 [N] (LN_ROW) / [M] (LN_COL)                                      */
  const float* ln_d;                  /* LN_COL only: f32 [M] added per output row                             */
  /* optional by-product: (mu, rstd) of every OUTPUT row (over its N columns, of the 16-bit-rounded values), for a
   * LayerNorm that follows -- out_stats = f32 [batch*M][2], eps = out_stats_eps.  NULL = none.  Not with GEGLU / OUT_F32. */
  float* out_stats; float out_stats_eps;
  /* Self-normalising LN_ROW: with ln_stats == NULL the GEMM computes (mu, rstd) of A's rows itself -- in the K loop of the
   * persistent kernel (two packed dot products per 16-B fragment chunk), by a statistics pass in front of the small-tile
   * kernels -- with eps = ln_eps; K must be the whole LayerNorm row (K % 8 == 0, K <= 1536), batch 1.  ln_stats_out
   * (f32 [M][2], or NULL) receives them, e.g. for the LN_COL projection of the same matrix that follows. */
  float ln_eps; float* ln_stats_out;
  /* Fused q | k | v projection (attention.py:168-172 -- to_q, to_k, to_v read the same LayerNorm output): with vt_out != NULL
   * the output columns n >= vt_col0 are stored TRANSPOSED, vt_out[(n - vt_col0) * ld_vt + m] (16-bit; ld_vt >= M, % 8 == 0)
   * -- the V^T[channel][token] image idf_attention consumes -- and `out` holds the first vt_col0 columns only.  Epilogue:
   * exactly LN_ROW (+ BIAS, which LN_ROW requires: the beta term of a transposed column is bias[n] as for the others);
   * anything else is IDF_E_ARG before any launch.  Batch 1, no out_stats; self-normalising LN_ROW additionally needs
   * ln_stats_out.  One launch of the persistent kernel when
   * N % 320 == vt_col0 % 320 == 0 and M % 16 == 0 (its transposed tiles run the same K loop with the MFMA operands swapped);
   * any other shape runs as the two GEMMs this replaces. */
  void* vt_out; int ld_vt; int vt_col0;
} idf_gemm_args;
int idf_gemm(const idf_gemm_args* a, void* stream);

/* ---- fused GEGLU feed-forward (attention.py:36-63 GEGLU / FeedForward; call sites :309 `x + tanh(alpha_dense) *
 * ff(norm2(x))` and :337 `ff(norm3(x)) + x`):  out = x + [gate[0] *] ( W2 . (value * gelu(gate)) + b2 ),
 * (value | gate) = LN(x) . W1^T + b1 -- ONE launch, the 4C-wide activated intermediate never leaves the CU (as two idf_gemm
 * calls it is written to and read back from HBM).  LayerNorm is folded as in IDF_EPI_LN_ROW: w1 carries gamma, ln_stats the
 * rows' (mu, rstd), cd the constants.  Operand images (packed once by the caller):
 *   w1  [8C][C]   rows interleaved [16 value | 16 gate] per 32 (IDF_EPI_GEGLU_P32's packing), ld = ldw1;
 *   cd  f32 [8C/64][128]: per 64 packed rows c[64] (row sums of the 16-bit w1) | d[64] (W1.beta + b1, packed like the rows);
 *   w2p [C][4C]   W2 with the k index permuted inside every 16-group: w2p[n][16 g + p] = W2[n][16 g + perm[p]],
 *                 perm = {0,1,2,3, 8,9,10,11, 4,5,6,7, 12,13,14,15}, ld = ldw2;
 * out may alias x.  Supported: C == 320 (the 64 x 64-latent blocks), M % 128 == 0; otherwise IDF_E_UNSUPPORTED and the
 * caller runs the two idf_gemm calls this replaces.  Results equal theirs up to the fp32 summation order of the second
 * product (the intermediate is rounded to the 16-bit type in both).                                                     */
typedef struct {
  const void* x; int ldx;
  const float* ln_stats;
  const void* w1; int ldw1;
  const float* cd;
  const void* w2p; int ldw2;
  const float* b2;
  const float* gate;                  /* device scalar, or NULL (= 1) */
  void* out; int ldo;
  int M, C;
  int dtype;
} idf_mlp_args;
int idf_mlp_geglu(const idf_mlp_args* a, void* stream);

/* (mu, rstd) of every row of a 16-bit [M, C] matrix (exact two-pass, fp32): stats[m] = (mean, 1/sqrt(var + eps)).
 * The stand-alone producer of `ln_stats` (idf_gemm's out_stats is the fused one).  C % 8 == 0, C <= 1536.          */
int idf_row_stats(const void* x, int ldx, float* stats, int M, int C, float eps, int dtype, void* stream);

/* ---- 3x3 convolution, pad 1, NHWC, implicit GEMM ---------------------------------------------------------
 * Replaces nn.Conv2d(k=3) call sites openaimodel.py:185,211 (ResBlock), :132-134 (Downsample, stride 2),
 * :98,107 (Upsample: nearest x2 folded into the gather), :463 (out conv).  W is [Cout][(ky*3+kx)*Cin + ci].
 * Cin % 64 == 0.  Output pixel rows m = (b, yo, xo).                                                        */
typedef struct {
  const void* x; const void* W; void* out;
  const float* bias; const void* rowbias; const void* res;
  int B, Hin, Win, Cin, Cout;
  int stride;       /* 1 or 2 */
  int upsample;     /* 0 or 1: input is nearest-upsampled x2 before the conv */
  int ldx, ldo, ldr, ld_rowbias;
  int n_valid;      /* OUT_NCHW: number of real output channels (<= Cout) */
  int epi; int dtype;
  void* ws; long long ws_bytes;       /* optional fp32 split-K workspace, as in idf_gemm_args */
  /* optional (ABI 5): GroupNorm(32) partial statistics of the OUTPUT as a by-product -- on return gn_partial holds, for every
   * sample b and 64-row chunk k of its Ho*Wo output rows, (mean, M2) per group: gn_partial[((b * (Ho*Wo/64) + k) * 32 + g) * 2],
   * i.e. exactly what idf_groupnorm_apply(.., nchunks = Ho*Wo/64) merges; the conv kernel leaves them from its epilogue
   * registers (no pass over the output) where it can, else the call runs the statistics pass itself.  Needs Ho*Wo % 64 == 0,
   * Cout % 32 == 0, ldo == Cout, a 16-bit NHWC output.  NULL = none.  (openaimodel.py:237-257: every ResBlock conv feeds a GroupNorm) */
  float* gn_partial;
} idf_conv3x3_args;
int idf_conv3x3(const idf_conv3x3_args* a, void* stream);
/* The VAE encoder's Downsample (ldm/modules/diffusionmodules/model.py:60-79): zero-pad RIGHT AND BOTTOM only, then 3x3 stride 2
 * without padding -- out[yo][xo] = sum w[ky][kx] x[2 yo + ky][2 xo + kx], rows / columns >= Hin / Win read zero,
 * Ho = (Hin - 2) / 2 + 1 (likewise Wo).  The same argument block, weight layout, epilogue flags, split-K workspace and gn_partial
 * contract as idf_conv3x3 (one launcher, the window origin moved by one pixel); stride must be 2, upsample 0, Hin, Win >= 2,
 * anything else is IDF_E_ARG before any launch.  Added within ABI 5: a new symbol only, no struct or existing entry point
 * changed, so callers built against the earlier ABI 5 header are unaffected. */
int idf_conv3x3_down(const idf_conv3x3_args* a, void* stream);
/* Upsample (openaimodel.py:98,107: F.interpolate(x, scale_factor=2, mode="nearest") then the 3x3 pad-1 conv) with the upsample
 * folded into the WEIGHTS instead of the gather: output pixel (2y + py, 2x + px) sees only a 2x2 window of the low-resolution image,
 * so the layer is four 2x2 convs (one per parity phase), 4 Cin multiply-adds per output instead of 9 Cin.
 *   W is [4][Cout][(ty*2+tx)*Cin + ci], phases in the order (py, px) = (0,0), (0,1), (1,0), (1,1); tap (ty, tx) of phase (py, px) reads
 *   x[y - 1 + py + ty][x - 1 + px + tx] (zero outside the image) and its weight is the sum of the 3x3 taps that land on that pixel:
 *   rows  py = 0: {ty 0: w[0], ty 1: w[1] + w[2]},  py = 1: {ty 0: w[0] + w[1], ty 1: w[2]};  columns likewise.
 *   (Sum the fp32 master weights and round to 16 bit once.)
 * The idf_conv3x3 argument block describing the layer it replaces: x [B, Hin, Win, Cin], out [B, 2 Hin, 2 Win, Cout] 16-bit NHWC,
 * stride 1, upsample 1, epi 0 or IDF_EPI_BIAS; rowbias, res, gn_partial NULL, n_valid 0 (else IDF_E_ARG); ws unused.
 * Runs on the persistent 256 x 320 kernel only (one launch, counted in IDF_STAT_GEMM_BIG_LAUNCHES): Cout % 320 == 0 and a tile
 * grid that passes its occupancy bar; any other shape returns IDF_E_UNSUPPORTED BEFORE any launch and the caller runs
 * idf_conv3x3(upsample = 1) with the 3x3 image.  Added within ABI 5 like idf_conv3x3_down: a new symbol only. */
int idf_conv_up2x_folded(const idf_conv3x3_args* a, void* stream);
/* ResBlock tail (openaimodel.py:237-257 with a 1x1 `skip_connection`): out = conv3x3(g) + Wskip . x + (b_conv + b_skip) as ONE
 * contraction over K = 9 C2 + Cx -- the shortcut runs as Cx / 64 extra K-tiles of the conv that read x at the output pixel itself,
 * instead of a GEMM that writes its 16-bit result to memory and a residual epilogue that reads it back.
 *   g [B, H, W, C2] (row stride ldg) is the conv input, x [B, H, W, Cx] (row stride ldx) the shortcut input; pad 1, stride 1.
 *   W is ONE image [Cout][9 C2 + Cx]: the conv taps (ky*3+kx)*C2 + ci first, then the Cx shortcut columns; bias (f32 [Cout], or NULL)
 *   is the SUM of the two layers' biases (add them in fp32 at pack time).  C2 % 64 == Cx % 64 == 0.
 *   out [B, H, W, Cout] 16-bit NHWC (row stride ldo); ws / ws_bytes: the optional fp32 split-K workspace of idf_conv3x3;
 *   gn_partial: idf_conv3x3's contract (statistics of the full output, shortcut included).
 * Runs on the persistent 256 x 320 kernel only (counted in IDF_STAT_GEMM_BIG_LAUNCHES and IDF_STAT_SKIP_FOLD_LAUNCHES): needs
 * Cout % 320 == 0 and a launch the dispatch rules of idf_conv3x3 would hand to that kernel; anything else returns
 * IDF_E_UNSUPPORTED BEFORE any launch and the caller runs idf_gemm + idf_conv3x3(res =) as before.  A null g / x / W / out, a
 * non-positive size, a C2 or Cx that is not a multiple of 64: IDF_E_ARG; a row stride % 8 or a pointer that is not 16-B aligned
 * (gn_partial: 8-B): IDF_E_ALIGN; all before any launch.  The shortcut does not pass through a 16-bit rounding here, so results differ
 * from the two-launch form by that rounding.  Added within ABI 5 like idf_conv_up2x_folded: a new symbol and a new struct only. */
typedef struct {
  const void* g; const void* x; const void* W; void* out;
  const float* bias;
  int B, H, Wd, C2, Cx, Cout;
  int ldg, ldx, ldo;
  int dtype;
  void* ws; long long ws_bytes;
  float* gn_partial;
} idf_conv3x3_skip_args;
int idf_conv3x3_skip(const idf_conv3x3_skip_args* a, void* stream);

/* first conv 4->C directly from the fp32 NCHW latent (openaimodel.py:371, :469-480): out NHWC 16-bit */
int idf_conv_in(const float* x_nchw, const float* w /*[C][Cin][3][3]*/, const float* bias, void* out,
                int B, int Cin, int H, int W, int Cout, int dtype, void* stream);

/* ---- fused multi-head attention (flash-style, online softmax) --------------------------------------------
 * Replaces F.scaled_dot_product_attention call sites attention.py:140,143 (cross), :263,266 (self / gated-self).
 * out[b][q][h*d + :] = softmax_j(Q.K_j / sqrt(d)) . V_j over TWO key/value segments (segment 1 may be empty):
 * the gated self-attention concatenates visual tokens and the 184 grounding tokens (attention.py:307) -- the
 * two-segment form never materialises the concatenation and only computes the N_visual query rows that
 * attention.py:308 keeps.  V is supplied TRANSPOSED: vt[b][h*d + e][j] (ld = ldv, padded to a multiple of 64).
 * d % 8 == 0, d <= 160, EXCEPT d = 104, 112, 136, 144 (7 or 9 K-steps of 16: the 32-query kernel has no instantiation for them),
 * which return IDF_E_UNSUPPORTED before any launch.
 * Optional instance-visibility mask (the reference's masked gated self-attention, attention.py:187-255, reached with
 * efficient_attention=False + grounding_input["att_masks"]): 32-bit words per query / per key; query q may attend key j
 * iff (qbits[b][q] & kbits{0,1}[b][j]) != 0, or j is q's own token in segment 0 (the reference's 1e-9 diagonal).
 * qbits == NULL (the default, all shipped configs) = no mask.  Strides in words per batch element.               */
typedef struct {
  const void* q; int ldq; long long strideQ; int nq;
  const void* k0; int ldk0; long long strideK0; const void* vt0; int ldv0; long long strideV0; int n0;
  const void* k1; int ldk1; long long strideK1; const void* vt1; int ldv1; long long strideV1; int n1;
  void* out; int ldo; long long strideO;
  int B, H, d;
  float scale;      /* d^-0.5 */
  int dtype;
  const void* qbits; long long strideQb;             /* [B][nq] u32, or NULL */
  const void* kbits0; long long strideKb0;           /* [B][n0] u32 */
  const void* kbits1; long long strideKb1;           /* [B][n1] u32 (when n1 > 0) */
} idf_attn_args;
int idf_attention(const idf_attn_args* a, void* stream);

/* ---- GroupNorm(32 groups) (+SiLU), fp32 statistics (util.py:223-226; attention.py:75-76) -----------------
 * x/out: [B, HW, C] 16-bit.  ws: f32 workspace of idf_groupnorm_ws_floats(B, HW) floats.                    */
long long idf_groupnorm_ws_floats(int B, int HW);
int idf_groupnorm(const void* x, void* out, const float* gamma, const float* beta, float* ws,
                  int B, int HW, int C, float eps, int silu, int dtype, void* stream);
/* The two halves of idf_groupnorm as separate calls (ABI 5): `partial` = [B][nchunks][32][2] fp32 (mean, M2) per (sample, row
 * chunk, group), chunk k = rows [k rpc, (k + 1) rpc), rpc = ceil(HW / nchunks).  idf_groupnorm_apply accepts the partials of
 * idf_groupnorm_stats or of a producer (idf_conv3x3's gn_partial, nchunks = HW / 64).  Bitwise run-to-run deterministic. */
int idf_groupnorm_stats(const void* x, float* partial, int B, int HW, int C, int nchunks, int dtype, void* stream);
int idf_groupnorm_apply(const void* x, void* out, const float* gamma, const float* beta, const float* partial,
                        int B, int HW, int C, int nchunks, float eps, int silu, int dtype, void* stream);

/* ---- LayerNorm over the last dim (attention.py:294-295,320-322), eps 1e-5 -------------------------------- */
int idf_layernorm(const void* x, int ldx, void* out, int ldo, const float* gamma, const float* beta,
                  int M, int C, float eps, int dtype, void* stream);

/* LayerNorm over C of an NHWC image whose output is written in 2x2/stride-2 PATCH order (row = (b, y/2, x/2),
 * column block ((y&1)*2+(x&1))*C, ld = ldo >= 4C): LayerNorm(channels_first) + the im2col of the 2x2 stride-2
 * downsample conv of ConvNeXt (convnext.py:78-82) in one pass, so that conv is a plain idf_gemm.               */
int idf_layernorm_patch2(const void* x, void* out, int ldo, const float* gamma, const float* beta,
                         int B, int H, int W, int C, float eps, int dtype, void* stream);

/* ---- UniFusion instance-mask tokenizer pieces (text_grounding_net.py:226-231; convnext.py:15-110), once per
 * conditioning.  idf_seg_in_conv: Conv2d(Cin<=32 -> 3, 3x3, pad 1) on fp32 [B,Cin,S,S], output written as the stem's
 * 4x4/stride-4 patch matrix out[b*(S/4)^2 + py*(S/4) + px][c*16 + ky*4 + kx] (16-bit, ld = ldo >= 48).
 * idf_dwconv7x7: depthwise 7x7 pad 3 on NHWC 16-bit; weights fp32 TAP-MAJOR [49][C].                             */
int idf_seg_in_conv(const float* segs, const float* w /*[3][Cin][3][3]*/, const float* bias, void* out,
                    int B, int Cin, int S, int ldo, int dtype, void* stream);
int idf_dwconv7x7(const void* x, const float* w_tap_major, const float* bias, void* out, int B, int H, int W, int C,
                  int dtype, void* stream);

/* ---- ScaleU (openaimodel.py:519-539 + Fourier_filter :25-48) ---------------------------------------------
 * out[b,p,0:Ch] = h * hscale[c];  out[b,p,Ch:Ch+Cs] = skip + sm1[0] * lowfreq4(skip)   (exact 4-bin identity)
 * hscale = tanh(scaleu_b)+1 (f32 [Ch]); sm1 = tanh(scaleu_s) (f32 scalar on device).
 * ws: f32 workspace of B*Cs*64 floats (8 row slices of partial plane sums); hscale 16-B aligned.            */
int idf_scaleu_concat(const void* h, const void* skip, void* out, const float* hscale, const float* sm1,
                      float* ws, int B, int H, int W, int Ch, int Cs, int dtype, void* stream);

/* ---- timestep embedding (util.py:160-180): out[b] = [cos(t f_k) | sin(t f_k)], k < dim/2 ----------------- */
int idf_timestep_embedding(const float* t, void* out, int B, int dim, int dtype, void* stream);

/* ---- UniFusion token-MLP input builder (text_grounding_net.py:216-287; util.py:12-26) --------------------
 * out[r][0:768]       = tmask[r] ? text[r] : null_text
 * out[r][768:768+32D] = lmask[r] ? fourier16(loc[r]) : null_loc       (sin/cos interleaved per frequency)   */
int idf_unifusion_embed(const float* text, const float* loc, const float* tmask, const float* lmask,
                        const float* null_text, const float* null_loc, const float* freqs /*[16]*/, void* out,
                        int rows, int text_dim, int D, int dtype, void* stream);

/* ---- samplers: fused CFG + PLMS update (plms.py:121-165) -------------------------------------------------
 * Both evaluate torch's fp32 expression with torch's operations in torch's order, every operation rounded to fp32 on its own (nothing
 * is contracted into an FMA, the divisions are the correctly rounded ones): the result equals the reference's tensor expression bit
 * for bit, and idf_cfg_combine's e_t is the e of idf_ddim_update on the same eps buffer.  Scalar accesses, one element per thread, any
 * 4-B aligned pointers; no synchronisation, no allocation; hipGraph-capturable.
 * idf_cfg_combine (plms.py:126):   e_t = eps_uncond + guidance * (eps_cond - eps_uncond)
 *   eps_cond / eps_uncond: the two halves of the engine's [cond | uncond] eps buffer (n floats each).  e_t must not overlap an input.
 *   IDF_E_ARG before any launch: a null pointer, n < 1.
 * idf_plms_update (plms.py:130-165 with sigma = 0), e' by mode, the sums left to right as written:
 *   0: e_t (the first step's predictor)   1: (e_t + e_next) / 2   2: (3 e_t - e1) / 2   3: (23 e_t - 16 e1 + 5 e2) / 12
 *   4: (55 e_t - 59 e1 + 37 e2 - 9 e3) / 24                   e1 / e2 / e3: the eps history, e1 the newest (old_eps[-1])
 *   pred_x0 = (x - sqrt_1m_at * e') / sqrt(a_t)               (:138)
 *   x_out   = sqrt(a_prev) * pred_x0 + sqrt(1 - a_prev) * e'  (:141-143)
 *   The three square roots are taken by the launcher in fp32 (sqrtf; the radicand 1 - a_prev is one fp32 subtraction), as the
 *   reference's torch.full(...) tensors are; sqrt_1m_at comes from the caller (the reference's ddim_sqrt_one_minus_alphas buffer).
 *   A pointer the mode does not read may be NULL and is never dereferenced.  x_out must not overlap an input.
 *   IDF_E_ARG before any launch: a null x / e_t / x_out, n < 1, mode outside 0..4, a null e_next in mode 1, a null e1 in modes 2-4, a
 *   null e2 in modes 3-4, a null e3 in mode 4, a_t <= 0, a_prev < 0, a_prev > 1, a non-finite a_t / a_prev / sqrt_1m_at.   */
int idf_cfg_combine(const float* eps_cond, const float* eps_uncond, float guidance, float* e_t,
                    long long n, void* stream);
int idf_plms_update(const float* x, const float* e_t, const float* e1, const float* e2, const float* e3,
                    const float* e_next, int mode, float a_t, float a_prev, float sqrt_1m_at,
                    float* x_out, long long n, void* stream);

/* ---- DDIM sampler: the per-step arithmetic around the UNet forward (ddim.py:94-98, :110-131; ldm.py:17-20) ----------------------
 * Both entry points were added within ABI 5: new symbols only, no struct or existing entry point changed.  Both evaluate torch's
 * fp32 expression with torch's operations in torch's order, every operation rounded to fp32 on its own (nothing is contracted into
 * an FMA, the division is the correctly rounded one): the result equals the reference's tensor expression bit for bit.  No
 * synchronisation, no allocation; hipGraph-capturable.  16-B accesses where every pointer is 16-B aligned and the vectors are
 * whole, scalar accesses otherwise (decided per launch).
 * idf_ddim_update = p_sample_ddim behind the model calls (ddim.py:110-131), one launch instead of idf_cfg_combine + an update:
 *   e       = eps_uncond + guidance * (eps_cond - eps_uncond)           (:114; eps_uncond == NULL: e = eps_cond, guidance unused)
 *   pred_x0 = (x - sqrt_1m_at * e) / sqrt(a_t)                          (:124)
 *   x_prev  = sqrt(a_prev) * pred_x0 + sqrt(1 - a_prev - sigma_t^2) * e (:127, :129)  [+ sigma_t * noise when noise != NULL (:128)]
 *   The three square roots are taken by the launcher in fp32, each operation rounded on its own, as the reference's
 *   torch.full(...) tensors are (:118-127).  eps_cond / eps_uncond: the two halves of the engine's [cond | uncond] eps buffer.
 *   x_prev may alias x; pred_x0 may be NULL (not stored).  IDF_E_ARG before any launch: a null x / eps_cond / x_prev, n < 1,
 *   a_t <= 0, a_prev < 0, sigma_t < 0, (1 - a_prev) - sigma_t^2 < 0, sigma_t != 0 with noise == NULL.
 * idf_q_sample_blend = q_sample (ldm.py:17-20) and the inpainting blend in front of a step (ddim.py:94-98; plms.py:99-104):
 *   out = (sqrt_ac * x0 + sqrt_1m_ac * noise) * mask + (1 - mask) * img
 *   x0, noise, img, out: [B][C][HW] fp32; mask: [B][1][HW] (mask_channels 1, broadcast over the channels) or [B][C][HW]
 *   (mask_channels C).  out may alias img.  IDF_E_ARG before any launch: a null pointer, B / C / HW < 1, mask_channels not 1 or C. */
int idf_ddim_update(const float* x, const float* eps_cond, const float* eps_uncond /* NULL = unguided */, float guidance,
                    float a_t, float a_prev, float sigma_t, float sqrt_1m_at, const float* noise /* NULL iff sigma_t == 0 */,
                    float* x_prev, float* pred_x0 /* or NULL */, long long n, void* stream);
int idf_q_sample_blend(const float* x0, const float* noise, const float* mask, const float* img, float sqrt_ac, float sqrt_1m_ac,
                       float* out, int B, int C, long long HW, int mask_channels /* 1 or C */, void* stream);
/* The same two launches over WORK UNITS (DDIMSamplerInst: the Multi-instance Sampler on DDIM steps).  Added within ABI 5: new symbols
 * only.  A forward of phase 1 advances U units, several of them trajectories of the same image; the per-image operands (the step
 * noise; the inpainting x0, its mask and its q_sample noise) stay [B] rows and are read through img_of: DEVICE int32 [U], unit u
 * belongs to image img_of[u].  The launcher cannot read the table: the kernel clamps every entry it loads to [0, B-1], so a wrong
 * table cannot send a load outside the per-image buffers.  Same device functions, same rounding, same access policy (16-B accesses
 * where every pointer is 16-B aligned and chw % 4 == 0 -- and HW % 4 == 0 under a channel-broadcast mask -- else scalar, decided per
 * launch); no allocation, no synchronisation; hipGraph-capturable; x_prev may alias x, out may alias img.
 * idf_ddim_update_units: x, eps_cond, eps_uncond, x_prev, pred_x0: [U][chw]; noise: [B][chw] or NULL (sigma_t == 0).  idf_ddim_update's
 *   expression with noise[img_of[u]] in place of noise[u].  img_of may be NULL when noise is NULL (nothing is per image) or when
 *   U == B (unit u is image u): the launch is then idf_ddim_update's own kernel, bit for bit.  IDF_E_ARG before any launch: every
 *   case of idf_ddim_update, U < 1, B < 1, chw < 1, noise != NULL with img_of == NULL and U != B.
 * idf_q_sample_blend_units: img, out: [U][C][HW]; x0, noise: [B][C][HW]; mask: [B][mask_channels][HW]; row img_of[u] of the three for
 *   unit u.  IDF_E_ARG before any launch: every case of idf_q_sample_blend, U < 1, B < 1, img_of == NULL. */
int idf_ddim_update_units(const float* x, const float* eps_cond, const float* eps_uncond /* NULL = unguided */, float guidance,
                          float a_t, float a_prev, float sigma_t, float sqrt_1m_at, const float* noise /* [B][chw]; NULL iff sigma_t == 0 */,
                          const int* img_of /* device int32 [U], or NULL */, float* x_prev, float* pred_x0 /* or NULL */, int U, int B,
                          long long chw, void* stream);
int idf_q_sample_blend_units(const float* x0, const float* noise, const float* mask, const float* img, const int* img_of,
                             float sqrt_ac, float sqrt_1m_ac, float* out, int U, int B, int C, long long HW,
                             int mask_channels /* 1 or C */, void* stream);

/* ---- entering the schedule part of the way: q_sample alone, and a resize of fp32 planes (host/hires.py: img2img starts and the latent
 * hi-res second pass).  Both were added within ABI 5: new symbols only.  No synchronisation, no allocation; hipGraph-capturable.
 * idf_q_sample = LatentDiffusion.q_sample (ldm.py:17-20) without a blend:
 *   out = sqrt_ac * x0 + sqrt_1m_ac * noise        fp32, each operation rounded on its own (nothing contracted): torch's expression bit
 *   for bit.  16-B accesses where x0, noise and out are 16-B aligned and n % 4 == 0, scalar accesses otherwise (decided per launch).
 *   out may alias x0.  IDF_E_ARG before any launch: a null pointer, n < 1, a non-finite coefficient.
 * idf_resize_planes: a separable resize of `planes` fp32 planes, src [planes][Hi][Wi] -> dst [planes][Ho][Wo], driven by DEVICE tables
 *   that the host builds in float64 (host/hires.resize_tables; torch's F.interpolate(align_corners=False) geometry from exact integer
 *   arithmetic): xi int32 [Wo] = the first source column of output column ox (may be negative: -2 at the leading outputs of a bicubic
 *   upscale), xw fp32 [Wo][taps] its weights; yi int32 [Ho]
 *   and yw fp32 [Ho][taps] likewise for the rows.  taps = 2 (bilinear) or 4 (bicubic).  The launcher cannot read the tables: the kernel
 *   clamps every idx + k to [0, n-1] where it becomes an address (also torch's border rule), so a wrong table cannot send a load
 *   outside src.  The expression is fixed, every operation rounded to fp32 on its own:
 *     row_j = ((s[r_j][c_0] * xw_0 + s[r_j][c_1] * xw_1) + s[r_j][c_2] * xw_2) + s[r_j][c_3] * xw_3
 *     out   = ((row_0 * yw_0 + row_1 * yw_1) + row_2 * yw_2) + row_3 * yw_3           (taps 2: the first two terms of each)
 *   Four outputs per thread along x; 16-B stores where Wo % 4 == 0 and dst is 16-B aligned, scalar stores otherwise (decided per
 *   launch); no LDS, no scratch.  dst must not overlap src.  IDF_E_ARG before any launch: a null pointer, a dimension < 1, taps not
 *   2 or 4, dst overlapping src; IDF_E_UNSUPPORTED: planes * Ho * Wo >= 2^31. */
int idf_q_sample(const float* x0, const float* noise, float sqrt_ac, float sqrt_1m_ac, float* out, long long n, void* stream);
int idf_resize_planes(const float* src, float* dst, const int* xi, const float* xw, const int* yi, const float* yw, int taps /* 2 or 4 */,
                      int planes, int Hi, int Wi, int Ho, int Wo, void* stream);

/* ---- DPM-Solver++(2M) step (Lu et al. 2022, "DPM-Solver++", Algorithm 2, data-prediction form) behind the UNet forward -------------
 * Added within ABI 5: a new symbol only.  The host computes the three step coefficients in float64 and rounds them to fp32 once
 * (host/samplers.dpmpp_coeffs); per element, every operation rounded to fp32 on its own (nothing contracted, correctly rounded division):
 *   e      = eps_uncond + guidance * (eps_cond - eps_uncond)            (eps_uncond == NULL: e = eps_cond, guidance unused)
 *   x0_out = (x - sqrt_1m_at * e) / sqrt_at                             the data prediction: the next step's x0_last
 *   x_prev = c_x * x + c_0 * x0_out  [+ c_1 * x0_last when x0_last != NULL: order 2]
 * Nothing in the step is per image, so there is no units variant.  16-B accesses where every pointer is 16-B aligned and n % 4 == 0,
 * scalar accesses otherwise (decided per launch); no LDS, no scratch, no allocation, no synchronisation; hipGraph-capturable.
 * x_prev may alias x, x0_out may alias x0_last (a thread reads its own elements before it writes them).  IDF_E_ARG before any
 * launch: a null x / eps_cond / x_prev / x0_out, n < 1, sqrt_at <= 0, a non-finite sqrt_at / sqrt_1m_at / c_x / c_0, a non-finite
 * c_1 with x0_last != NULL. */
int idf_dpmpp_update(const float* x, const float* eps_cond, const float* eps_uncond /* NULL = unguided */, float guidance,
                     float sqrt_at, float sqrt_1m_at, float c_x, float c_0, float c_1,
                     const float* x0_last /* NULL = order 1; then c_1 is not used */,
                     float* x_prev, float* x0_out /* required: the next step's history */, long long n, void* stream);

/* ---- Multi-instance Sampler merge (plms_instance.py:112-135) ---------------------------------------------
 * lat: [n_inst+1][B][C][H][W] fp32.  mode 0: mean over the first dim; mode 1: crop-and-paste of instance j's
 * latent box (boxes: int32 [n_inst][4] = int(box*latent_size), reference index order dim2<-x, dim3<-y).
 * Torch's fp32 result bit for bit, each operation rounded on its own:
 *   mode 0: s = 0.f; for k = 0 .. n_inst, in order: s += lat[k]; out = s / (float)(n_inst + 1)        (:135)
 *   mode 1: lat[0], then for k = 1 .. n_inst, in order, out[:, :, b0:b2, b1:b3] = lat[k][:, :, b0:b2, b1:b3] with (b0, b1, b2, b3) =
 *           boxes[k-1]: dim 2 (H) sliced with b0:b2, dim 3 (W) with b1:b3, later instances win (:112-132).  A box may be empty or
 *           inverted (nothing is pasted) and may reach past H or W (clipped); its coordinates must be >= 0 (a negative index
 *           counts from the end in the reference's slices; here it would count from row or column 0).
 * boxes: DEVICE int32, read in mode 1 only.  out must not overlap lat.  Scalar accesses, one element per thread; no allocation, no
 * synchronisation; hipGraph-capturable.  IDF_E_ARG before any launch: a null lat / out, n_inst < 0, a non-positive B / C / H / W,
 * mode not 0 or 1, mode 1 with boxes == NULL.      */
int idf_mis_merge(const float* lat, const int* boxes, float* out, int n_inst, int B, int C, int H, int W,
                  int mode, void* stream);
/* The same merge over a RAGGED unit list: a batch of images with different instance counts (PLMSSamplerInst.sample_layouts), one
 * launch for the whole batch.  Added within ABI 5: a new symbol only.  lat: [U][C][H][W] fp32, the unit latents image after image;
 * unit_off: DEVICE int32 [B+1], image b owns the units unit_off[b] .. unit_off[b+1]-1 and the first of them is its global
 * (full-conditioning) trajectory; out: [B][C][H][W].
 *   mode 0: s = 0.f; for k in image b's units, in order: s += lat[k]; out = s / (float)count   (idf_mis_merge's operation order,
 *           each operation rounded on its own: equal counts give idf_mis_merge's result bit for bit)
 *   mode 1: the global unit, then every later unit of the image overwrites its latent box (boxes: int32 [U][4], the entry of a
 *           global unit is ignored; dim 2 sliced with box[0]:box[2], dim 3 with box[1]:box[3], later units win)
 * No allocation, no synchronisation; hipGraph-capturable.  16-B accesses where lat and out are 16-B aligned and C*H*W % 4 == 0,
 * scalar accesses otherwise (decided per launch).  The launcher cannot read the table: the kernel clamps every offset it loads
 * to [0, U], so a wrong table cannot send a load outside lat; an image left without units is written as zeros.  IDF_E_ARG before
 * any launch: a null lat / unit_off / out, B < 1, U < B, a non-positive dimension, mode not 0 or 1, mode 1 with boxes == NULL. */
int idf_mis_merge_ragged(const float* lat, const int* unit_off, const int* boxes /* mode 1, else NULL */, float* out, int B, int U,
                         int C, int H, int W, int mode, void* stream);

/* ---- VAE decoder pieces (AutoencoderKL.decode, the step right after the sampling path) --------
 * idf_softmax_rows: p[r][0:n] = softmax(scale * s[r][0:n]) for `rows` stacked rows (row r at s + r*lds / p + r*ldp);
 * s fp32, p 16-bit.  Replaces the torch.bmm -> softmax of the single-head 512-channel AttnBlock
 * (ldm/modules/diffusionmodules/model.py:185-189): the scores come from idf_gemm(.., IDF_EPI_OUT_F32), this kernel
 * normalises them, a second idf_gemm applies V (:194).  n % 4 == 0, lds % 4 == 0, ldp % 4 == 0, scale > 0.
 * idf_pointwise_nchw: 1x1 conv between small channel counts (Cin <= 16) on fp32 NCHW, input pre-scaled by in_scale:
 * AutoencoderKL.decode's `1/scale_factor * z` + post_quant_conv (ldm/models/autoencoder.py:32-35).  bias may be NULL.
 * One rounding of in_scale * x, then Cin FMAs from the bias.  IDF_E_ARG before any launch: a null x / w / out, Cin > 16, a non-positive
 * B / Cin / Cout / HW.
 * (The decoder's other layers are idf_conv_in / idf_groupnorm / idf_conv3x3 / idf_gemm calls.)                          */
int idf_softmax_rows(const float* s, void* p, long long rows, int n, long long lds, long long ldp, float scale,
                     int dtype, void* stream);
int idf_pointwise_nchw(const float* x, const float* w /*[Cout][Cin]*/, const float* bias, float* out, int B, int Cin,
                       int Cout, long long HW, float in_scale, void* stream);

/* ---- VAE encoder tail (ldm/models/autoencoder.py:27-31, ldm/modules/distributions/distributions.py:24-37) -------------
 * One launch for everything behind the encoder's conv_out: h = fp32 NCHW [B, C2, H, W] (what IDF_EPI_OUT_NCHW writes),
 * moments = quant_conv(h) with w [2E][C2], bias f32 [2E] or NULL (C2 <= 16, 2E <= 16), (mean | logvar) = channel halves,
 * logvar clamped to [-30, 20], z[B, E, H, W] = (mean + exp(0.5 logvar) * noise) * scale in fp32.  noise == NULL gives the mode
 * (z = mean * scale).  moments != NULL additionally receives [B, 2E, H, W] (mean | clamped logvar).  HW = H * W.  (The encoder's
 * other layers are idf_conv_in / idf_groupnorm / idf_conv3x3 / idf_conv3x3_down / idf_gemm / idf_softmax_rows calls.)
 * Added within ABI 5 like idf_conv3x3_down: a new symbol only. */
int idf_vae_posterior(const float* h, const float* w /*[2E][C2]*/, const float* bias, const float* noise, float scale, float* z,
                      float* moments, int B, int C2, int E, long long HW, void* stream);

/* ---- CLIP text transformer (ldm/modules/encoders/modules.py:144-172: FrozenCLIPEmbedder.forward -> CLIPTextModel) ---------------
 * Its other layers are idf_gemm (LayerNorm folded in with self-computed statistics, BIAS / RES / IDF_EPI_QUICKGELU epilogues) and
 * idf_layernorm calls.  Both entry points were added within ABI 5: new symbols only.
 * idf_attention_causal: qkv = the 16-bit row-major output of the fused projection, rows b*T + t, columns [q | k | v], each block H*d
 * wide, ld >= 3*H*d;  out[b*T + t][h*d + :] = softmax_{j <= t}(scale * q_t . k_j) . v_j  (ldo >= H*d).  One workgroup per (b, h) with
 * K and V^T of the head resident in LDS, both products on 16x16x32 MFMA, fp32 online softmax, P rounded to the 16-bit type before
 * P.V; rows <= p do not depend on anything at positions > p bit for bit.  Supported: d == 64, 1 <= T <= 128; anything else is
 * IDF_E_UNSUPPORTED, a row start that is not 16-B aligned (ld % 8, ldo % 8, the pointers) IDF_E_ALIGN, before any launch.
 * idf_clip_embed: out[b*T + t][0:C] = tok_emb[ids[b][t]][0:C] + pos_emb[t][0:C] (fp32 sum, one rounding); ids int32 [B][T], tok_emb
 * 16-bit [vocab][C], pos_emb 16-bit [>= T][C], both contiguous; an id outside [0, vocab) is clamped into it.  C % 8 == 0. */
int idf_attention_causal(const void* qkv, int ld, void* out, int ldo, int B, int T, int H, int d, float scale, int dtype, void* stream);
int idf_clip_embed(const int* ids, const void* tok_emb, const void* pos_emb, void* out, int ldo, int B, int T, int C, int vocab,
                   int dtype, void* stream);

/* ---- CLIP image tower (eval/eval_attribute_binding.py:19-60: CLIPModel.get_image_features -> CLIPVisionTransformer) ------------------
 * A ViT layer is the text layer with bidirectional attention; the other launches are idf_gemm / idf_layernorm.  Both entry points
 * were added within ABI 5: new symbols only.
 * idf_attention_qkv: the argument list and the qkv layout of idf_attention_causal;
 * out[b*T + t][h*d + :] = softmax_j(scale * q_t . k_j) . v_j over ALL j < T.  Same kernel design (K and V^T of the head resident in
 * LDS, here dynamic and sized by T: (ceil32(T) * 72 + 64 * (ceil32(T) + 4)) * 2 bytes, 78848 at the maximum).  Supported: d == 64 and
 * 1 <= T <= IDF_ATTENTION_QKV_TMAX = 288 (ViT-L/14 at 224 px has T = 257; the 336-px model's T = 577 does not fit); anything else is
 * IDF_E_UNSUPPORTED, a row start that is not 16-B aligned IDF_E_ALIGN, ld < 3*H*d / ldo < H*d / T < 1 / B < 1 IDF_E_ARG, all
 * before any launch.  Keys in [T, ceil32(T)) are zero-filled in LDS and masked by select; nothing is read behind row B*T.
 * idf_clip_patchify: pixels fp32 NCHW [B][3][S][S] -> patches 16-bit [B*G*G][ldp >= Kp], G = S / P, Kp = 3*P*P rounded up to a
 * multiple of 64: patches[(b*G + gy)*G + gx][c*P*P + ky*P + kx] = pixels[b][c][gy*P + ky][gx*P + kx] (the column order of the
 * flattened patch_embedding.weight [C][3][P][P]), one rounding, columns [3*P*P, Kp) zero.  The same launch writes the class rows
 * x[b*(G*G + 1)][0:C] = cls_row[0:C] (16-bit; x has ldx >= C).  The patch rows of x then come from one batched idf_gemm
 * (batch = B, M = G*G, strideA = G*G*ldp, out = x + ldx, strideO = (G*G + 1)*ldx, IDF_EPI_RES with res = position rows 1.., strideR =
 * 0).  S % P == 0, P <= 32, else IDF_E_ARG; C % 8, ldp % 8, ldx % 8 and 16-B aligned 16-bit pointers, else IDF_E_ALIGN. */
#define IDF_ATTENTION_QKV_TMAX 288
int idf_attention_qkv(const void* qkv, int ld, void* out, int ldo, int B, int T, int H, int d, float scale, int dtype, void* stream);
int idf_clip_patchify(const float* pixels, void* patches, int ldp, const void* cls_row, void* x, int ldx, int B, int S, int P, int C,
                      int dtype, void* stream);

/* ---- CLIP preprocessing on the device (host/clip_score.py: crop_instances + preprocess; eval/eval_attribute_binding.py:186-190 and
 * the CLIPFeatureExtractor behind it).  Added within ABI 5: a new symbol and new enum values only.
 * idf_clip_crop_resize: one launch turns a batch of source images and a list of crops into the image tower's input,
 *   out fp32 [Ncrop][3][S][S] = (v / 255 - mean) / std of the crop, bicubic-resized so that its short side is S and centre-cropped to
 *   S x S, BIT FOR BIT what Pillow's Image.resize(BICUBIC) gives: its 8-bit resample is two integer passes,
 *   clip8((2^21 + sum pixel * k) >> 22) in int32, horizontal then vertical on the uint8 result, over coefficient tables that the
 *   HOST builds in float64 (host/clip_score.resample_tables) -- the kernel evaluates no filter and no fp32 expression that could round.
 * src, by `kind`: IDF_CLIP_SRC_U8 uint8 [B][H][W][3] (what a PNG holds), or IDF_CLIP_SRC_F32 fp32 [B][3][H][W] (what
 *   AutoencoderKL.decode returns; finite values), quantised on the way in as inference.save_images does: clamp to [-1, 1],
 *   * 0.5 + 0.5, * 255 in fp32, truncation.
 * crops: HOST memory, int32 [Ncrop][8] = (image b, x0, y0, width, height, table set t, 0, 0), the rectangle inside the image; checked
 *   here, before any launch.
 * tables: DEVICE memory, int32, three blocks: the same Ncrop crop records; then per table set [2 axes][S][2] = (first, count) of every
 *   output index of the S-wide window (axis 0 horizontal, 1 vertical; first counts from the crop's corner); then per table set
 *   [2 axes][K][S] coefficients, tap-major, zero behind an index' count.  Crops of one size share a table set (Ntab <= Ncrop).
 *   K = the largest Pillow ksize of the call, 2 ceil(support) + 1 (11 for 512 -> 224).
 * lut: DEVICE fp32 [3][256], channel c / byte v -> output value (host/clip_score.pixel_lut).
 * IDF_E_ARG: a null pointer, B / H / W / Ncrop / Ntab / S / K < 1, S % 4, Ncrop > 65535, an unknown kind, a crop record outside its
 *   image or table range; IDF_E_UNSUPPORTED: K > IDF_CLIP_RESIZE_KMAX = 32 (a 1024-px short side resized to 224 needs 21), or an S
 *   whose band of intermediate rows does not fit the kernel's 48 KB of LDS at K taps; IDF_E_ALIGN: out not 16-B aligned, tables /
 *   lut / fp32 src not 4-B aligned.  All before any launch (IDF_STAT_CLIP_PREPROC_LAUNCHES counts the launches).  Device table
 *   entries are clamped wherever they become an address. */
enum { IDF_CLIP_SRC_U8 = 0, IDF_CLIP_SRC_F32 = 1 };
#define IDF_CLIP_RESIZE_KMAX 32
int idf_clip_crop_resize(const void* src, int kind, int B, int H, int W, const int* crops, int Ncrop, const int* tables, int Ntab,
                         const float* lut, float* out, int S, int K, void* stream);

/* ---- instance masks on the device (host/masks.py; the reference decodes COCO RLE with pycocotools and resizes with Pillow NEAREST on
 * the host, utils/input.py:161-186).  Added within ABI 5: a new symbol only.
 * idf_rle_decode_planes: M jobs, one launch.  Job m decodes the run-length mask whose CUMULATIVE run ends are
 *   ends[run_begin[m] .. run_end[m]) (uint32, runs alternate 0, 1, 0, .. over the column-major pixel index p = x * h + y of the
 *   h x w = src_hw[m][0] x src_hw[m][1] source; zero-length runs are legal; a p behind the last end reads 0) and writes plane
 *   dst_plane[m] of out (fp32 [P][S][S]) in full: out[plane][Y][X] = 0.0f / 1.0f, the value of source pixel sy = ((2Y + 1) h) / (2S),
 *   sx = ((2X + 1) w) / (2S) in integer arithmetic -- Pillow's Image.resize((S, S), NEAREST).  Planes no job names are not touched.
 *   area[m] (int32 [M]) is INCREMENTED by the number of ones job m wrote: the caller zeroes it.  Several jobs may share one run range.
 * All tables are DEVICE memory and cannot be read here: the host validates them (host/masks.pack_masks); the kernel checks every
 *   entry where it becomes an address, and a job with run_begin < 0, run_begin > run_end, run_end > n_ends, dst_plane outside [0, P),
 *   h or w < 1, h * w >= 2^31 or S * max(h, w) >= 2^31 writes nothing.
 * IDF_E_ARG: a null pointer, M < 0, n_ends < 0, P < 1, S < 1; IDF_E_UNSUPPORTED: S % 4, P * S * S >= 2^31, M > 65535; IDF_E_ALIGN: out
 *   not 16-B aligned, a table not 4-B aligned.  All before any launch; M == 0 launches nothing and returns 0. */
int idf_rle_decode_planes(const unsigned* ends, int n_ends, const int* run_begin, const int* run_end, const int* src_hw,
                          const int* dst_plane, int M, float* out, int P, int S, int* area, void* stream);

/* ---- layout helpers ---------------------------------------------------------------------------------------*/
int idf_cast_f32_to_16(const float* x, void* out, long long n, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IDF_H_ */
