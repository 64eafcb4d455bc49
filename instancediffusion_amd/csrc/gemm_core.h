// gemm_core.h -- pieces shared by the MFMA GEMM / implicit-GEMM conv translation units (gemm_conv.hip, gemm_big.hip):
// the launch parameter block, the K-tile depth, the device pieces every K-loop kernel of the family uses unchanged (tile order and
// decode, conv gather rules, LDS-DMA source rows, the fragment-read + MFMA body of a K-tile) and the 8-column epilogue.  The
// schedules -- each kernel's order of loads, waits, barriers and computes -- stay in the kernels' own files.
#pragma once
#include "common.h"
#include <atomic>

namespace idfcore {

struct CoreParams {
  const unsigned short* W; int ldw; long long strideW; int N;
  const unsigned short* A; int lda; long long strideA; int M; int K;
  int Hin, Win, Cin, Ho, Wo, stride, up;           // conv gather
  void* out; int ldo; long long strideO;
  const float* bias; const unsigned short* rowbias; int ld_rowbias; int rows_per_batch;
  const unsigned short* res; int ldr; long long strideR;
  const float* gate; int epi; int n_valid;
  float* ws; size_t ws_bytes; int splitk; int kt_per_slice;   // split-K: fp32 partial slabs ws[slice][tail_rows][N]
  // hybrid split (persistent kernel): work items [0, full_items) are whole tiles (kt_full K-tiles, normal epilogue); the
  // remaining tiles -- rows [tail_m0, tail_m0 + tail_rows) -- are cut into `splitk` K-slices each.  Uniform split-K:
  // full_items = 0, tail_m0 = 0, tail_rows = M.
  int full_items; int kt_full; int tail_m0; int tail_rows;
  // LayerNorm folded into the GEMM (IDF_EPI_LN_ROW / IDF_EPI_LN_COL, include/idf.h): (mu, rstd) pairs of the normalised
  // operand's rows, the column sums c of the gamma-folded weight and (LN_COL) the beta term d
  const float* ln_stats; long long stride_ln_stats; const float* ln_c; const float* ln_d;
  // LN_ROW with ln_stats == nullptr: the kernel computes (mu, rstd) of A's rows itself (eps = ln_eps) and, when
  // ln_stats_out != nullptr, leaves them there ([M][2]) for an LN_COL consumer of the same matrix
  float ln_eps; float* ln_stats_out;
  // fused q | k | v projection: output columns n >= vt_col0 are stored transposed, vt_out[(n - vt_col0) * ld_vt + m]
  unsigned short* vt_out; int ld_vt; int vt_col0;
  // out_stats by-product of the persistent kernel: every wave leaves (mean, M2) of the BN/2 output columns it owns of a row
  // in stat_parts[(m * parts + tile_n * 2 + wn) * 2 ..] (fp32, workspace); stats_finalize merges the `parts` slots of a row
  float* stat_parts; int parts;
  // GroupNorm partials of the output as a by-product of the persistent kernel's conv epilogue (round 5): (mean, M2) per
  // (sample, 64-row chunk, group) in gn_partial[sample][gn_hw / 64][32][2]; gn_hw = rows per sample
  float* gn_partial; int gn_hw;
  // persistent-kernel schedule (round 4; every setting computes the same bits), set by launch_big_cfg alone: tile_walk 0 =
  // strided, 1 = chunked; dephase = P start groups per XCD (always 0: off), dephase_units = one tile's estimated duration in
  // units of 1024 cycles; epi_vmcnt (always 1): the first K-tile behind an epilogue waits with a counted vmcnt (the epilogue's
  // stores drain under it).  The two constants are arguments because of what the compiler makes of the kernel without them
  int tile_walk; int dephase; int dephase_units; int epi_vmcnt;
  // conv gather: zero rows / columns in front of the image (the window origin is yo * stride - pad_lo).  1 = the symmetric
  // pad 1 of idf_conv3x3; 0 = idf_conv3x3_down (the VAE encoder's Downsample pads right and bottom only).  Wave-uniform.
  int pad_lo;
  // folded nearest-x2 upsample (gemm_kernel_big<.., FOLD>, idf_conv_up2x_folded): tiles of ONE output parity phase; work item
  // `tile` belongs to phase tile / fold_tiles.  M, Ho, Wo describe the low-resolution image (one phase), W holds four images.
  int fold_tiles;
  // ResBlock 1x1 shortcut as extra K-tiles of the 3x3 conv (gemm_kernel_big<.., SKIPK>, idf_conv3x3_skip): K = 9 Cin + Cx; the
  // K-tiles from 9 Cin on read Cx channels of A2 (row stride lda2) at the OUTPUT pixel itself -- a tenth "tap" without padding
  const unsigned short* A2; int lda2; int Cx;
};

constexpr int BK = 64;

// ================================================================================================================
// K-loop core.  Everything is __forceinline__ with its sizes as template parameters or arguments that are constants at the call
// site, so it folds into the calling kernel exactly as the code it replaced (profiles/gemm_shared_core.md).
// ================================================================================================================
// XCD-aware tile order: workgroup L of T runs on XCD L % 8 (8 private L2s); give each XCD a CONTIGUOUS chunk of the n-fastest
// tile list so the n-tiles that share one activation m-tile hit the same L2 (bijective for any count).
__device__ __forceinline__ int xcd_tile(int L, int T) {
  const int q = T >> 3, r = T & 7, xcd = L & 7, i = L >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}
// tile of the n-fastest list -> its origin, the operands of its batch entry (blockIdx.z; split-K launches are never batched) and
// the K-tiles [kt_begin, kt_begin + nk) of this block's K-slice (blockIdx.z of a split-K launch).  Filled through the reference:
// returned by value, gemm_kernel_ring's kernel-argument loads come out in another order.
struct TileSlice { int m0, n0, bz; const unsigned short* Wb; const unsigned short* Ab; int kt_begin, nk; };
template <int BM, int BN>
__device__ __forceinline__ void tile_slice(const CoreParams& p, int tile, TileSlice& t) {
  const int tiles_n = (p.N + BN - 1) / BN;
  const int m_tile = tile / tiles_n;
  t.n0 = (tile - m_tile * tiles_n) * BN, t.m0 = m_tile * BM;
  t.bz = (p.splitk > 1) ? 0 : blockIdx.z;
  t.Wb = p.W + (size_t)t.bz * p.strideW;
  t.Ab = p.A + (size_t)t.bz * p.strideA;
  const int nk_all = p.K / BK;
  t.kt_begin = (p.splitk > 1) ? blockIdx.z * p.kt_per_slice : 0;
  t.nk = (p.splitk > 1) ? min(p.kt_per_slice, nk_all - t.kt_begin) : nk_all;
}

// ---- conv gather.  Output row m = (sample b, output pixel yo, xo); its 3x3 window starts at (ay, ax) of the (upsampled) image
struct ConvPixel { int b, yo, xo; };
__device__ __forceinline__ ConvPixel conv_pixel(const CoreParams& p, int m) {
  const int hw = p.Ho * p.Wo;
  const int b = m / hw, rem = m - b * hw;
  const int yo = rem / p.Wo;
  return {b, yo, rem - yo * p.Wo};
}
// window origin of row m (pre-multiplied by stride, minus the leading pad); returns the element offset of the row's image
__device__ __forceinline__ size_t conv_row_origin(const CoreParams& p, int m, int& ay, int& ax) {
  const ConvPixel px = conv_pixel(p, m);
  ay = px.yo * p.stride - p.pad_lo;
  ax = px.xo * p.stride - p.pad_lo;
  return (size_t)px.b * p.Hin * p.Win * p.lda;
}
// K element k_elem -> (3x3 tap, first input channel); the step to the next K-tile of `bk` elements; is pixel (yi, xi) of the tap
// inside the Hup x Wup image (else it is zero padding)
__device__ __forceinline__ void conv_tap_at(const CoreParams& p, int k_elem, int& tap, int& ci0) {
  tap = k_elem / p.Cin;
  ci0 = k_elem - tap * p.Cin;
}
__device__ __forceinline__ void conv_tap_step(const CoreParams& p, int bk, int& tap, int& ci0) {
  ci0 += bk;
  if (ci0 >= p.Cin) { ci0 = 0; ++tap; }
}
// ... and with the tenth source behind the nine taps (CoreParams::A2): K elements from 9 Cin on are "tap 9", whose Cx channels may
// be more or fewer than Cin, so the tap index saturates there and ci0 runs on to Cx (the K-tile stream of an output tile ends with it)
__device__ __forceinline__ void conv_tap_at_skip(const CoreParams& p, int k_elem, int& tap, int& ci0) {
  tap = min(k_elem / p.Cin, 9);
  ci0 = k_elem - tap * p.Cin;
}
__device__ __forceinline__ void conv_tap_step_skip(const CoreParams& p, int bk, int& tap, int& ci0) {
  ci0 += bk;
  if (tap < 9 && ci0 >= p.Cin) { ci0 = 0; ++tap; }
}
__device__ __forceinline__ bool conv_tap_inside(int yi, int xi, int Hup, int Wup) { return (yi >= 0) & (yi < Hup) & (xi >= 0) & (xi < Wup); }

// ---- LDS-DMA tile image of the 4-wave kernels: linear 128-B rows (64 elements); instruction j of a wave covers tile rows
// 8 * (wave + 4 j) .. + 7, lane -> (row lane >> 3, 16-B slot lane & 7); the slot is XOR-swizzled on the SOURCE side (slot c of LDS
// row `row` holds global chunk c ^ ((row >> 1) & 7)) and, identically, on the fragment reads (ktile_mfma): conflict-free ds_read_b128
__device__ __forceinline__ int dma_row(int wave, int j, int lane) { return 8 * (wave + 4 * j) + (lane >> 3); }
__device__ __forceinline__ int dma_chunk(int row, int lane) { return ((lane & 7) ^ ((row >> 1) & 7)) * 8; }
// per-lane source of instruction j of a dense operand tile: rows r0 .. of the [rows][ld] matrix `base` (rows beyond the matrix
// are clamped duplicates), from element k0 of the row
__device__ __forceinline__ const unsigned short* dma_src_row(const unsigned short* base, int ld, int r0, int rows, size_t k0, int wave,
                                                             int j, int lane) {
  const int row = dma_row(wave, j, lane);
  const int n = min(r0 + row, rows - 1);
  return base + (size_t)n * ld + k0 + dma_chunk(row, lane);
}
// ... and of all INST instructions of the tile (gemm_kernel_dma calls dma_src_row from its own loop: through this form its
// register allocation moves, 123 -> 108 and 63 -> 68 VGPRs)
template <int INST>
__device__ __forceinline__ void dma_src_rows(const unsigned short* (&src)[INST], const unsigned short* base, int ld, int r0, int rows,
                                             size_t k0, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < INST; ++j) src[j] = dma_src_row(base, ld, r0, rows, k0, wave, j, lane);
}

template <int TN, int TM>
__device__ __forceinline__ void clear_acc(f32x16 (&acc)[TN][TM]) {
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
}
// One K-tile: acc[a][b] += W fragment a . A fragment b over the BK / 16 K-steps.  wf_base / af_base = the lane's row (l31) of the
// wave's weight / activation rows in the LDS image of row stride RS elements; hi = lane >> 5 selects the 16-B half of a K-step;
// SWZ: the 16-B slot is XOR-swizzled with f_sw = (l31 >> 1) & 7 (fragment rows are (multiple of 32) + l31).
// The fragment reads of K-step ks+1 are issued BEFORE the MFMAs of K-step ks (register double-buffer), so the LDS latency (~100+
// cycles) hides under 4-8 MFMAs instead of stalling every K-step (the compiler does not do this).
template <int DT, int TN, int TM, int RS, bool SWZ>
__device__ __forceinline__ void ktile_mfma(f32x16 (&acc)[TN][TM], const unsigned short* wf_base, const unsigned short* af_base, int hi,
                                           int f_sw) {
  u32x4 wf[2][TN], af[2][TM];
  {
    const int slot = SWZ ? (hi ^ f_sw) * 8 : hi * 8;
#pragma unroll
    for (int a = 0; a < TN; ++a) wf[0][a] = *reinterpret_cast<const u32x4*>(wf_base + a * 32 * RS + slot);
#pragma unroll
    for (int b = 0; b < TM; ++b) af[0][b] = *reinterpret_cast<const u32x4*>(af_base + b * 32 * RS + slot);
  }
#pragma unroll
  for (int ks = 0; ks < BK / 16; ++ks) {
    const int cur = ks & 1, nxt = cur ^ 1;
    if (ks + 1 < BK / 16) {
      const int slot = SWZ ? (((ks + 1) * 2 + hi) ^ f_sw) * 8 : (ks + 1) * 16 + hi * 8;
#pragma unroll
      for (int a = 0; a < TN; ++a) wf[nxt][a] = *reinterpret_cast<const u32x4*>(wf_base + a * 32 * RS + slot);
#pragma unroll
      for (int b = 0; b < TM; ++b) af[nxt][b] = *reinterpret_cast<const u32x4*>(af_base + b * 32 * RS + slot);
    }
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int b = 0; b < TM; ++b) acc[a][b] = Elem<DT>::mfma32(wf[cur][a], af[cur][b], acc[a][b]);
  }
}

// Epilogue for 8 consecutive output columns n..n+7 of row m (n % 8 == 0).  Shared by the main kernel (after the
// accumulators were transposed through LDS so that a lane owns a contiguous 8-column run -> 16-B coalesced residual /
// rowbias loads and FULL-LINE 16-B stores) and by the split-K reducer.
template <int DT>
__device__ __forceinline__ void epilogue8(const CoreParams& p, int bz, int m, int n, float* v, float gate) {
  const int epi = p.epi;
  const bool full = (n + 7 < p.N);
  if (epi & IDF_EPI_LN_ROW) {                       // v = rstd_m * (acc - mu_m * c[n]); the beta term arrives as bias
    const f32x2 st = *reinterpret_cast<const f32x2*>(p.ln_stats + (size_t)bz * p.stride_ln_stats + 2 * (size_t)m);
#pragma unroll
    for (int e = 0; e < 8; ++e) if (n + e < p.N) v[e] = st[1] * fmaf(-st[0], p.ln_c[n + e], v[e]);
  }
  if (epi & IDF_EPI_LN_COL) {                       // v = rstd_n * (acc - c[m] * mu_n) + d[m]
    const float cm = p.ln_c[m], dm = p.ln_d[m];
    const float* st = p.ln_stats + (size_t)bz * p.stride_ln_stats + 2 * (size_t)n;
#pragma unroll
    for (int e = 0; e < 8; ++e) if (n + e < p.N) v[e] = fmaf(st[2 * e + 1], fmaf(-cm, st[2 * e], v[e]), dm);
  }
  if (epi & IDF_EPI_BIAS) {
    if (full) {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + n), b1 = *reinterpret_cast<const f32x4*>(p.bias + n + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] += b0[e]; v[e + 4] += b1[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (n + e < p.N) v[e] += p.bias[n + e];
    }
  }
  if (epi & IDF_EPI_ROWBIAS) {
    const unsigned short* rb = p.rowbias + (size_t)(m / p.rows_per_batch) * p.ld_rowbias + n;
    if (full && ((p.ld_rowbias & 7) == 0)) {
      float r[8];
      unpack8<DT>(*reinterpret_cast<const u32x4*>(rb), r);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += r[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (n + e < p.N) v[e] += Elem<DT>::to_f32(rb[e]);
    }
  }
  if (epi & IDF_EPI_SILU) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
  }
  if (epi & IDF_EPI_GELU) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = gelu_erf_f(v[e]);
  }
  if (epi & IDF_EPI_QUICKGELU) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = quick_gelu_f(v[e]);
  }
  if (epi & IDF_EPI_RES) {
    const unsigned short* rr = p.res + (size_t)bz * p.strideR + (size_t)m * p.ldr + n;
    const float gm = (epi & IDF_EPI_GATE) ? gate : 1.0f;
    if (full && ((p.ldr & 7) == 0)) {
      float r[8];
      unpack8<DT>(*reinterpret_cast<const u32x4*>(rr), r);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(gm, v[e], r[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (n + e < p.N) v[e] = fmaf(gm, v[e], Elem<DT>::to_f32(rr[e]));
    }
  }
  if (epi & IDF_EPI_OUT_NCHW) {
    const int hw = p.Ho * p.Wo;
    const int bb = m / hw, rem = m - bb * hw;
    float* o = reinterpret_cast<float*>(p.out);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (n + e < p.n_valid) o[((size_t)bb * p.n_valid + (n + e)) * hw + rem] = v[e];
  } else if (epi & IDF_EPI_OUT_F32) {
    float* o = reinterpret_cast<float*>(p.out) + (size_t)bz * p.strideO + (size_t)m * p.ldo + n;
    if (full && ((p.ldo & 3) == 0)) {
      *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (n + e < p.N) o[e] = v[e];
    }
  } else {
    unsigned short* o = reinterpret_cast<unsigned short*>(p.out) + (size_t)bz * p.strideO + (size_t)m * p.ldo + n;
    if (full && ((p.ldo & 7) == 0)) {
      *reinterpret_cast<u32x4*>(o) = pack8<DT>(v);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (n + e < p.N) o[e] = Elem<DT>::from_f32(v[e]);
    }
  }
}

}  // namespace idfcore

// Big-tile persistent kernel (gemm_big.hip).  Returns IDF_BIG_UNSUPPORTED when the shape does not qualify.
#define IDF_BIG_UNSUPPORTED (-100)
extern std::atomic<long long> idf_stat_big_launches;     // process-global launch counter (idf_get_stat)
// *splitk_out > 1 on return: the kernel left fp32 partials of that many K-slices in p.ws; the caller runs the reducer
// *parts_out (optional): > 0 when the kernel left per-wave partial output-row statistics in p.stat_parts (p.stat_parts
// offered and the launch was an unsplit dense GEMM), the number of slots per row.
// *gst_out (optional): 1 when the kernel left the GroupNorm partials of its output in p.gn_partial (see CoreParams).
int idf_launch_big(const idfcore::CoreParams& p, int dtype, bool conv, bool force, hipStream_t s, int* splitk_out,
                   int* parts_out = nullptr, int* tail_m0_out = nullptr, int* gst_out = nullptr);
// nearest-x2 upsample + 3x3 conv as four 2x2 phase convs in one persistent launch (see idf_conv_up2x_folded, include/idf.h);
// IDF_BIG_UNSUPPORTED = the shape does not qualify (nothing launched).  `force` skips the occupancy bar as in idf_launch_big.
int idf_launch_big_fold(const idfcore::CoreParams& p, int dtype, bool force, hipStream_t s);
int idf_launch_qkv320w(const idfcore::CoreParams& p, int dtype, hipStream_t s);   // qkv_fused.hip; IDF_BIG_UNSUPPORTED = not its shape
int idf_launch_geglu640w(const idfcore::CoreParams& p, int dtype, hipStream_t s);   // geglu_fused.hip; IDF_BIG_UNSUPPORTED = not its shape
int idf_gegluw_set_mode(int v);                         // 0 = never, 1 = when the shape qualifies; returns the previous mode
int idf_launch_qkv640w(const idfcore::CoreParams& p, int dtype, hipStream_t s);   // qkv640_fused.hip
int idf_qkvw_set_mode(int v);                           // both levels; 0 = never, 1 = when the shape qualifies; returns the previous mode
int idf_launch_proj320s(const idfcore::CoreParams& p, int dtype, float* out_stats, float out_stats_eps, hipStream_t s);   // proj320_stream.hip; writes final out_stats itself
int idf_projw_set_mode(int v);                          // 0 = never, 1 = when the shape qualifies; returns the previous mode
int idf_projw_min_rows();                               // least M proj320s_kernel takes on the current device (two 256-row tiles per CU); 0 = knob off
int idf_mlp_set_mode(int v);                            // mlp_fused.hip: 0 = mlp320_kernel, 1 = mlp320w_kernel; returns the previous mode
int idf_big_min_eff_pct(int set);                        // automatic rule's occupancy bar in per cent (set < 0: query)
int idf_num_cu();                                        // CUs of the current device (cached)
// (mu, rstd) per row from `parts` equal-count (mean, M2) slots per row (fixed merge order): out_stats[m] = f32x2
int idf_stats_finalize(const float* stat_parts, int parts, int cols_per_part, float* out_stats, int M, float eps, hipStream_t s);
