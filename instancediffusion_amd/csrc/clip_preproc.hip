// clip_preproc.hip -- idf_clip_crop_resize: the stretch between "the decoder wrote an image" and "the CLIP image tower sees S x S
// pixels" (host/clip_score.py: crop_instances + preprocess) in one launch, bit for bit what Pillow computes.  gfx950 only.
//
// Pillow's 8-bit bicubic resample (ImagingResample) is integer arithmetic once its coefficient tables exist: a pass is
// clip8((2^21 + sum pixel * k) >> 22) in int32, the horizontal pass first, the vertical pass on its uint8 result.  The tables come
// from the host (host/clip_score.resample_tables: float64, Pillow's summation order) -- device code contracts a * b + c to an FMA
// and the cubic would stop matching -- and so does the last step, (v / 255 - mean) / std, as a 3 x 256 fp32 table.
//
// One 256-thread workgroup per (crop, band of R output rows):
//   1. horizontal pass over exactly the intermediate rows the band's vertical taps need, [first(r0), first(r1 - 1) + count(r1 - 1)),
//      window columns only: a thread owns one (row, column) and its three channels, lanes run along x (neighbouring lanes read
//      neighbouring source pixels of one row).  The fp32 source kind is quantised on the way in by the rule of inference.save_images:
//      clamp to [-1, 1], * 0.5 + 0.5 (exact, or rounded as the two separate operations round: x * 0.5 is exact), * 255 as a lone
//      multiply, truncate.  The rows go to LDS as uint8 planes [row][channel][S], never to HBM;
//   2. vertical pass from LDS: a thread owns four neighbouring columns of one (row, channel) -- one dword read per tap, four int32
//      accumulators -- looks the four bytes up in the pixel table (staged in LDS) and stores 16 B of out[n][c][r][x .. x + 3].
// The crop record and the band bounds are workgroup-uniform loads (SGPRs).  R comes from K: the band's intermediate rows number at
// most (R - 1) * scale + 2 * support + 1 <= (R - 1) (K - 1) / 4 + K, as K = 2 ceil(support) + 1 and scale <= support / 2.
// Every table entry is clamped where it becomes an address (source pixel, LDS row, tap count), so a table that does not belong to
// its crop gives wrong pixels, never an access outside the image, the tables or the LDS image.
#include "common.h"

std::atomic<long long> idf_stat_clip_preproc_launches{0};   // idf_clip_crop_resize launches (idf_get_stat)

namespace {

constexpr int CR_PRECISION = 22;                  // Pillow's PRECISION_BITS for 8-bit data
constexpr int CR_LUT_BYTES = 3 * 256 * 4;
constexpr int CR_LDS_BUDGET = 48 * 1024;          // three workgroups per CU
constexpr int CR_BAND_MAX = 16;

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> CR_PRECISION;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// inference.save_images: clamp(x, -1, 1) * 0.5 + 0.5, then * 255 in fp32 and truncation
__device__ __forceinline__ int quantise(float v) {
  v = fminf(fmaxf(v, -1.0f), 1.0f);
  v = v * 0.5f + 0.5f;
  return (int)__fmul_rn(v, 255.0f);
}

// the host's rows of the bound for R output rows at K taps
inline int band_rows(int R, int K) { return ((R - 1) * (K - 1) + 3) / 4 + K; }

template <int KIND>
__global__ __launch_bounds__(256) void clip_crop_resize_kernel(const void* __restrict__ src, int B, int H, int W, const int* __restrict__ tab,
                                                               int Ncrop, int Ntab, const float* __restrict__ lut, float* __restrict__ out,
                                                               int S, int K, int R, int cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cr_lds[];
  float* lut_s = reinterpret_cast<float*>(cr_lds);
  unsigned char* mid = cr_lds + CR_LUT_BYTES;                 // [cap][3][S] uint8
  const int tid = threadIdx.x;
  const int n = blockIdx.y, r0 = blockIdx.x * R;
  const int r1 = min(r0 + R, S);
  // workgroup-uniform: the crop record (image, corner, table set) and the band's intermediate rows
  const int* rec = tab + (size_t)n * 8;
  const int b = clampi(rec[0], 0, B - 1), x0 = rec[1], y0 = rec[2], t = clampi(rec[5], 0, Ntab - 1);
  const int* bounds = tab + (size_t)Ncrop * 8 + (size_t)t * 4 * S;               // [2][S][2]: (first, count)
  const int* coef = tab + (size_t)Ncrop * 8 + (size_t)Ntab * 4 * S + (size_t)t * 2 * K * S;   // [2][K][S]: tap-major
  const int* hb = bounds, * vb = bounds + 2 * S;
  const int* hc = coef, * vc = coef + (size_t)K * S;
  const int ylo = vb[2 * r0];                                 // first and first + count do not decrease along the axis
  const int nrows = clampi(vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1] - ylo, 1, cap);

  for (int i = tid; i < 3 * 256; i += 256) lut_s[i] = lut[i];

  for (int i = tid; i < nrows * S; i += 256) {
    const int row = i / S, x = i - row * S;
    const int f = x0 + hb[2 * x], cnt = min(hb[2 * x + 1], K);
    const int sy = clampi(y0 + ylo + row, 0, H - 1);
    int a0 = 1 << (CR_PRECISION - 1), a1 = a0, a2 = a0;
    if constexpr (KIND == IDF_CLIP_SRC_U8) {
      const unsigned char* line = static_cast<const unsigned char*>(src) + ((size_t)b * H + sy) * W * 3;
      for (int k = 0; k < cnt; ++k) {
        const int w = hc[k * S + x];
        const unsigned char* p = line + (size_t)clampi(f + k, 0, W - 1) * 3;
        a0 += p[0] * w;
        a1 += p[1] * w;
        a2 += p[2] * w;
      }
    } else {
      const size_t plane = (size_t)H * W;
      const float* line = static_cast<const float*>(src) + (size_t)b * 3 * plane + (size_t)sy * W;
      for (int k = 0; k < cnt; ++k) {
        const int w = hc[k * S + x];
        const float* p = line + clampi(f + k, 0, W - 1);
        a0 += quantise(p[0]) * w;
        a1 += quantise(p[plane]) * w;
        a2 += quantise(p[2 * plane]) * w;
      }
    }
    unsigned char* m = mid + (size_t)row * 3 * S + x;
    m[0] = (unsigned char)clip8(a0);
    m[S] = (unsigned char)clip8(a1);
    m[2 * S] = (unsigned char)clip8(a2);
  }
  __syncthreads();

  const int S4 = S >> 2, per_row = 3 * S4;
  for (int i = tid; i < (r1 - r0) * per_row; i += 256) {
    const int r = i / per_row, rem = i - r * per_row, c = rem / S4, x4 = rem - c * S4;
    const int rr = r0 + r;
    const int f = vb[2 * rr] - ylo, cnt = min(vb[2 * rr + 1], K);
    int a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = 1 << (CR_PRECISION - 1);
    const unsigned char* col = mid + c * S + x4 * 4;
    for (int k = 0; k < cnt; ++k) {
      const int w = vc[k * S + rr];
      const unsigned p = *reinterpret_cast<const unsigned*>(col + (size_t)clampi(f + k, 0, nrows - 1) * 3 * S);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += (int)((p >> (8 * j)) & 0xffu) * w;
    }
    const float* l = lut_s + c * 256;
    const f32x4 o = {l[clip8(a[0])], l[clip8(a[1])], l[clip8(a[2])], l[clip8(a[3])]};
    *reinterpret_cast<f32x4*>(out + (((size_t)n * 3 + c) * S + rr) * S + x4 * 4) = o;
  }
}

}  // namespace

extern "C" int idf_clip_crop_resize(const void* src, int kind, int B, int H, int W, const int* crops, int Ncrop, const int* tables, int Ntab,
                                    const float* lut, float* out, int S, int K, void* stream) {
  if (!src || !crops || !tables || !lut || !out || B <= 0 || H <= 0 || W <= 0 || Ncrop <= 0 || Ncrop > 65535 || Ntab <= 0) return IDF_E_ARG;
  if (S <= 0 || (S % 4) || K <= 0 || (kind != IDF_CLIP_SRC_U8 && kind != IDF_CLIP_SRC_F32)) return IDF_E_ARG;
  if (K > IDF_CLIP_RESIZE_KMAX) return IDF_E_UNSUPPORTED;
  for (int n = 0; n < Ncrop; ++n) {
    const int* r = crops + (size_t)n * 8;                     // (image, x0, y0, width, height, table set, 0, 0)
    if (r[0] < 0 || r[0] >= B || r[1] < 0 || r[2] < 0 || r[3] <= 0 || r[4] <= 0 || r[5] < 0 || r[5] >= Ntab) return IDF_E_ARG;
    if ((long long)r[1] + r[3] > W || (long long)r[2] + r[4] > H) return IDF_E_ARG;
  }
  if (!aligned16(out) || (((uintptr_t)tables) & 3u) || (((uintptr_t)lut) & 3u) || (kind == IDF_CLIP_SRC_F32 && (((uintptr_t)src) & 3u)))
    return IDF_E_ALIGN;
  int R = S < CR_BAND_MAX ? S : CR_BAND_MAX;
  while (R > 1 && (long long)band_rows(R, K) * 3 * S > CR_LDS_BUDGET - CR_LUT_BYTES) --R;
  const int cap = band_rows(R, K);
  if ((long long)cap * 3 * S > CR_LDS_BUDGET - CR_LUT_BYTES) return IDF_E_UNSUPPORTED;     // S too large for K taps even at one row
  const int smem = CR_LUT_BYTES + cap * 3 * S;
  const dim3 grid((unsigned)((S + R - 1) / R), (unsigned)Ncrop);
  hipStream_t s = (hipStream_t)stream;
  if (kind == IDF_CLIP_SRC_U8)
    hipLaunchKernelGGL(clip_crop_resize_kernel<IDF_CLIP_SRC_U8>, grid, dim3(256), smem, s, src, B, H, W, tables, Ncrop, Ntab, lut, out, S, K, R, cap);
  else
    hipLaunchKernelGGL(clip_crop_resize_kernel<IDF_CLIP_SRC_F32>, grid, dim3(256), smem, s, src, B, H, W, tables, Ncrop, Ntab, lut, out, S, K, R, cap);
  idf_stat_clip_preproc_launches.fetch_add(1);
  return idf_launch_status();
}
