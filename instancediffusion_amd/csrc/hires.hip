// hires.hip -- idf_resize_planes: separable bilinear / bicubic resize of fp32 planes (the latents between the two passes of a hi-res
// run, host/hires.py).  gfx950 only.
//
// The kernel evaluates no filter and no source coordinate: the HOST builds, in float64 from exact integer arithmetic
// (host/hires.resize_tables), per output column its first tap xi[ox] (may be negative) and `taps` fp32 weights xw[ox][taps], and the same per
// output row (yi, yw).  The launcher cannot read those device tables, so every tap index idx + k is clamped to [0, n-1] where it becomes
// an address -- which is also torch's border rule (upsample_bicubic2d / upsample_bilinear2d read the clamped neighbour).
//
// The expression is fixed, every operation rounded to fp32 on its own (nothing contracted into an FMA), so that a torch fp32 restatement
// equals the result bit for bit:
//   row_j = ((s[r_j][c_0] xw_0 + s[r_j][c_1] xw_1) + s[r_j][c_2] xw_2) + s[r_j][c_3] xw_3
//   out   = ((row_0 yw_0 + row_1 yw_1) + row_2 yw_2) + row_3 yw_3                                  (taps 2: the first two terms of each)
//
// Bandwidth-bound and plain: one thread per RESIZE_X neighbouring outputs of one row (one 16-B store when Wo % 4 == 0 and dst is 16-B
// aligned, scalar stores with a tail guard otherwise), lanes along x so that a wave's stores are contiguous; the thread's column
// weights, column indices and row weights are loaded once; the source taps are plain loads that hit L2 / the vector cache (a 64^2
// plane is 16 KB and every element is read by ~taps^2 (Wo Ho) / (Wi Hi) threads).  No LDS, no scratch.
#include "common.h"

namespace {

constexpr int RESIZE_X = 4;                       // outputs per thread along x

template <int TAPS, bool VEC>
__global__ __launch_bounds__(256) void resize_planes_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            const int* __restrict__ xi, const float* __restrict__ xw,
                                                            const int* __restrict__ yi, const float* __restrict__ yw, unsigned threads,
                                                            int Hi, int Wi, int Ho, int Wo, int XG) {
#pragma clang fp contract(off)
  static_assert(TAPS == 2 || TAPS == 4, "bilinear or bicubic");
  const unsigned i = blockIdx.x * 256u + threadIdx.x;                                 // threads <= planes Ho Wo < 2^31: 32-bit divisions
  if (i >= threads) return;
  const unsigned row = i / (unsigned)XG;                                              // plane * Ho + oy
  const int xg = (int)(i - row * (unsigned)XG);
  const unsigned plane = row / (unsigned)Ho;
  const int oy = (int)(row - plane * (unsigned)Ho);
  const int ox0 = xg * RESIZE_X;
  const float* __restrict__ sp = src + (long long)plane * ((long long)Hi * Wi);

  // the thread's tables, loaded once.  A first tap is clamped to [-TAPS, n-1] before the tap offset is added: that changes no clamped
  // idx + k and keeps the sum inside int for any table content.
  int col[RESIZE_X][TAPS];
  float wx[RESIZE_X][TAPS];
#pragma unroll
  for (int j = 0; j < RESIZE_X; ++j) {
    const int ox = min(ox0 + j, Wo - 1);                                              // the tail of a scalar row recomputes its last column
    const int first = min(max(xi[ox], -TAPS), Wi - 1);
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
      col[j][k] = min(max(first + k, 0), Wi - 1);
      wx[j][k] = xw[(long long)ox * TAPS + k];
    }
  }
  const int rfirst = min(max(yi[oy], -TAPS), Hi - 1);
  float acc[RESIZE_X];
#pragma unroll
  for (int r = 0; r < TAPS; ++r) {
    const int rr = min(max(rfirst + r, 0), Hi - 1);
    const float wy = yw[(long long)oy * TAPS + r];
    const float* __restrict__ srow = sp + (long long)rr * Wi;
#pragma unroll
    for (int j = 0; j < RESIZE_X; ++j) {
      float h = srow[col[j][0]] * wx[j][0];
#pragma unroll
      for (int k = 1; k < TAPS; ++k) {
        const float t = srow[col[j][k]] * wx[j][k];
        h = h + t;
      }
      const float v = h * wy;
      acc[j] = r == 0 ? v : acc[j] + v;
    }
  }
  float* __restrict__ dp = dst + (long long)row * Wo + ox0;
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(dp) = f32x4{acc[0], acc[1], acc[2], acc[3]};             // Wo % 4 == 0: whole vectors, 16-B aligned
  } else {
#pragma unroll
    for (int j = 0; j < RESIZE_X; ++j)
      if (ox0 + j < Wo) dp[j] = acc[j];
  }
}

}  // namespace

extern "C" int idf_resize_planes(const float* src, float* dst, const int* xi, const float* xw, const int* yi, const float* yw, int taps,
                                 int planes, int Hi, int Wi, int Ho, int Wo, void* stream) {
  if (!src || !dst || !xi || !xw || !yi || !yw) return IDF_E_ARG;
  if (planes < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || (taps != 2 && taps != 4)) return IDF_E_ARG;
  const long long n_in = (long long)planes * Hi * Wi, n_out = (long long)planes * Ho * Wo;
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)n_in * 4u, d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)n_out * 4u;
  if (s0 < d1 && d0 < s1) return IDF_E_ARG;                                           // dst overlaps src
  if (n_out >= (1ll << 31)) return IDF_E_UNSUPPORTED;
  const int XG = (Wo + RESIZE_X - 1) / RESIZE_X;
  const unsigned threads = (unsigned)((long long)planes * Ho * XG);                   // <= n_out < 2^31
  const bool vec = (Wo % 4) == 0 && aligned16(dst);
  const dim3 grid((threads + 255u) / 256u);
  hipStream_t s = (hipStream_t)stream;
#define IDF_RESIZE_LAUNCH(T, V) \
  hipLaunchKernelGGL((resize_planes_kernel<T, V>), grid, dim3(256), 0, s, src, dst, xi, xw, yi, yw, threads, Hi, Wi, Ho, Wo, XG)
  if (taps == 4) { if (vec) IDF_RESIZE_LAUNCH(4, true); else IDF_RESIZE_LAUNCH(4, false); }
  else { if (vec) IDF_RESIZE_LAUNCH(2, true); else IDF_RESIZE_LAUNCH(2, false); }
#undef IDF_RESIZE_LAUNCH
  return idf_launch_status();
}
