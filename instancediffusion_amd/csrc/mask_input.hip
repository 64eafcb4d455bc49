// mask_input.hip -- idf_rle_decode_planes: COCO run-length masks -> the fp32 {0, 1} planes of the `segs` conditioning stacks, decoded
// and nearest-resized to S x S in one launch (host/masks.py: parse_rle + pack_masks build the tables, decode_rle_reference is the
// CPU twin).  Only the run lengths cross PCIe; the 1 MB planes are written once, on the device.  gfx950 only.
//
// A mask of h x w pixels is a list of runs over the COLUMN-MAJOR pixel index p = x * h + y, alternating 0, 1, 0, ..; the host hands
// over the cumulative run ends, so pixel p lies in run #{i : ends[i] <= p} and its value is that number's parity (behind the last
// end: 0).  Output pixel (Y, X) reads source pixel sy = ((2Y + 1) h) / (2S), sx = ((2X + 1) w) / (2S) -- Pillow's NEAREST, integer
// for integer.
//
// One 256-thread workgroup per (job, band of RLE_BAND output rows).  A thread owns four neighbouring X (one 16-B store per row,
// lanes along X: a wave's stores of one row are 1 KB contiguous) and walks a sub-band of rows downwards: at fixed X consecutive Y
// walk one source column, p only grows, so each of the four columns is searched once (upper bound by bisection, the four searches in
// lock step) and then stepped, the current run's end held in a register.  The job's ends sit in LDS when they fit RLE_LDS_RUNS entries, else the
// same search runs on global memory.  `area` is reduced per wave by shuffles, per workgroup in LDS, then one atomic add.
// Every table entry is checked where it becomes an address: a job whose run range, destination plane or source size is out of
// range writes nothing.
#include "common.h"

namespace {

constexpr int RLE_BAND = 32;                      // output rows per workgroup: at S = 512 a thread walks 16 rows per search
constexpr int RLE_LDS_RUNS = 4096;                // 16 KB of cumulative ends (the demo masks have 121 .. 1153 runs): 8 workgroups per CU

// idx[j] = #{i in [0, n) : e[i] <= p[j]}: the run that holds pixel p[j].  Four bisections in lock step -- their loads are independent,
// so a step costs one LDS (or global) round trip for all four; `steps` = bit length of n, wave-uniform.
template <typename Ends>
__device__ __forceinline__ void runs_of4(Ends e, int n, int steps, const unsigned* p, int* idx) {
  int lo[4] = {0, 0, 0, 0}, hi[4] = {n, n, n, n};
  for (int s = 0; s < steps; ++s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (lo[j] < hi[j]) {                          // mid < hi <= n
        const int mid = (lo[j] + hi[j]) >> 1;
        if (e[mid] <= p[j]) lo[j] = mid + 1; else hi[j] = mid;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = lo[j];
}

template <typename Ends>
__device__ __forceinline__ int decode_band(Ends e, int n, unsigned h, unsigned w, int S, int r0, int r1, float* __restrict__ plane) {
  const int XG = S >> 2;
  int nsub = 256 / XG;
  nsub = nsub < 1 ? 1 : (nsub > r1 - r0 ? r1 - r0 : nsub);
  const int rs = (r1 - r0 + nsub - 1) / nsub;
  const unsigned S2 = 2u * (unsigned)S;
  const int steps = n > 0 ? 32 - __builtin_clz((unsigned)n) : 0;      // a range of n entries is empty after that many halvings
  int ones = 0;
  for (int i = threadIdx.x; i < XG * nsub; i += 256) {
    const int sub = i / XG, xg = i - sub * XG;
    const int ya = r0 + sub * rs, yb = min(ya + rs, r1);
    if (ya >= yb) continue;
    unsigned base[4];
    int idx[4];
    const unsigned sy0 = ((2u * ya + 1u) * h) / S2;
    unsigned p0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      base[j] = (((2u * (unsigned)(xg * 4 + j) + 1u) * w) / S2) * h;
      p0[j] = base[j] + sy0;
    }
    runs_of4(e, n, steps, p0, idx);
    unsigned end[4];                                 // where the column's current run ends: no load per row until p crosses it
#pragma unroll
    for (int j = 0; j < 4; ++j) end[j] = idx[j] < n ? e[idx[j]] : 0xffffffffu;       // p < 2^31 never reaches the sentinel
    for (int Y = ya; Y < yb; ++Y) {
      const unsigned sy = ((2u * Y + 1u) * h) / S2;
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned p = base[j] + sy;
        while (p >= end[j]) {
          ++idx[j];
          end[j] = idx[j] < n ? e[idx[j]] : 0xffffffffu;
        }
        const int bit = (idx[j] < n) ? (idx[j] & 1) : 0;
        ones += bit;
        o[j] = bit ? 1.0f : 0.0f;
      }
      *reinterpret_cast<f32x4*>(plane + (size_t)Y * S + xg * 4) = o;
    }
  }
  return ones;
}

__global__ __launch_bounds__(256) void rle_decode_planes_kernel(const unsigned* __restrict__ ends, int n_ends, const int* __restrict__ run_begin,
                                                                const int* __restrict__ run_end, const int* __restrict__ src_hw,
                                                                const int* __restrict__ dst_plane, float* __restrict__ out, int P, int S,
                                                                int* __restrict__ area) {
  __shared__ unsigned ends_s[RLE_LDS_RUNS];
  __shared__ int ones_s[4];
  const int m = blockIdx.y, r0 = blockIdx.x * RLE_BAND;
  const int r1 = min(r0 + RLE_BAND, S);
  // workgroup-uniform job record; every field is checked before it becomes an address
  const int rb = run_begin[m], re = run_end[m], plane = dst_plane[m], h = src_hw[2 * m], w = src_hw[2 * m + 1];
  if (rb < 0 || re < rb || re > n_ends || plane < 0 || plane >= P || h <= 0 || w <= 0) return;
  const unsigned long long big = (unsigned long long)(h > w ? h : w) * (unsigned long long)S;
  if ((unsigned long long)h * (unsigned long long)w >= (1ull << 31) || big >= (1ull << 31)) return;   // (2S - 1) h and p stay in 32 bits
  const int n = re - rb;
  const unsigned* e = ends + rb;
  float* dst = out + (size_t)plane * S * S;
  int ones;
  if (n <= RLE_LDS_RUNS) {
    for (int i = threadIdx.x; i < n; i += 256) ends_s[i] = e[i];
    __syncthreads();
    ones = decode_band(static_cast<const unsigned*>(ends_s), n, (unsigned)h, (unsigned)w, S, r0, r1, dst);
  } else {
    ones = decode_band(e, n, (unsigned)h, (unsigned)w, S, r0, r1, dst);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o, 64);
  if ((threadIdx.x & 63) == 0) ones_s[threadIdx.x >> 6] = ones;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = ones_s[0] + ones_s[1] + ones_s[2] + ones_s[3];
    if (total) atomicAdd(area + m, total);
  }
}

}  // namespace

extern "C" int idf_rle_decode_planes(const unsigned* ends, int n_ends, const int* run_begin, const int* run_end, const int* src_hw,
                                     const int* dst_plane, int M, float* out, int P, int S, int* area, void* stream) {
  if (M < 0 || P <= 0 || S <= 0 || n_ends < 0) return IDF_E_ARG;
  if (!ends || !run_begin || !run_end || !src_hw || !dst_plane || !out || !area) return IDF_E_ARG;
  if (S % 4 || (long long)P * S * S >= (1ll << 31) || M > 65535) return IDF_E_UNSUPPORTED;
  if (!aligned16(out) || (((uintptr_t)ends | (uintptr_t)run_begin | (uintptr_t)run_end | (uintptr_t)src_hw | (uintptr_t)dst_plane |
                           (uintptr_t)area) & 3u))
    return IDF_E_ALIGN;
  if (M == 0) return 0;
  const dim3 grid((unsigned)((S + RLE_BAND - 1) / RLE_BAND), (unsigned)M);
  hipLaunchKernelGGL(rle_decode_planes_kernel, grid, dim3(256), 0, (hipStream_t)stream, ends, n_ends, run_begin, run_end, src_hw, dst_plane,
                     out, P, S, area);
  return idf_launch_status();
}
