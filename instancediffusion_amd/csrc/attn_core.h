// attn_core.h -- what the attention translation units share (attention.hip, attention4.hip, attention4w.hip, attention8.hip):
// the parameter block, the device pieces that every kernel of the family uses unchanged (LDS-DMA primitives, block order, tile
// bookkeeping, tail source rules, the normalise-and-store epilogue) and the launchers' common host checks and prototypes.  The
// schedules -- each kernel's tile loop and its qk / exp_pack / pv lambdas -- stay in the kernels' own files.
#pragma once
#include "common.h"
#include <cstdlib>

namespace idfattn {

struct AttnParams {
  const unsigned short* q; int ldq; long long sQ; int nq;
  const unsigned short* k[2]; int ldk[2]; long long sK[2];
  const unsigned short* vt[2]; int ldv[2]; long long sV[2]; int n[2];
  unsigned short* out; int ldo; long long sO;
  int H, d;
  float scale_log2;   // d^-0.5 * log2(e)
  // optional instance-visibility mask (masked gated self-attention, reference attention.py:187-255): query q may attend
  // key j iff (qbits[q] & kbits[seg][j]) != 0, or j is q's own token in segment 0.  NULL qbits = no mask.
  const unsigned* qbits; long long sQb;
  const unsigned* kbits[2]; long long sKb[2];
};


// ================================================================================================================
// Device section.  Everything is __forceinline__ with its sizes as template parameters or arguments that are constants at the
// call site, so it folds into the calling kernel exactly as the code it replaced.
// ================================================================================================================
constexpr int KVT = 64;            // keys per tile, in every kernel of the family

// The bf16 / fp16 ones page (source of the softmax-denominator row) of an LDS-DMA kernel; like the zero page (IDF_ZERO_PAGE,
// common.h, next to the LDS-DMA primitives) every file that needs one defines its own through this.
#define IDF_ATTN_ONES_PAGE(name)                                                                        \
  __device__ __attribute__((aligned(16))) unsigned short name[2][8] = {                                 \
      {0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80},      /* bf16 1.0 */            \
      {0x3c00, 0x3c00, 0x3c00, 0x3c00, 0x3c00, 0x3c00, 0x3c00, 0x3c00}}      /* fp16 1.0 */

__device__ __forceinline__ float max3f(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// maximum / sum over the two lane halves (hi = lane >> 5) that share a query
__device__ __forceinline__ float half_max(float mx, int hi) {
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
  return fmaxf(mx, __uint_as_float(hi ? sw[0] : sw[1]));
}
__device__ __forceinline__ float half_sum(float v, int hi) {
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return v + __uint_as_float(hi ? sw[0] : sw[1]);
}

// ---- XCD-aware block order: hardware block L of `total` runs on XCD L % 8 and every XCD has its own L2; this gives every XCD a
// contiguous range of logical blocks, so the query blocks of one (batch, head) share one L2 with their K / V^T.
__device__ __forceinline__ int xcd_block(int L, int total, bool on) {
  if (on && (total & 7) == 0) L = (L & 7) * (total >> 3) + (L >> 3);
  return L;
}
// logical block L of the 1-D grids -> (query block, head, batch), query blocks fastest
__device__ __forceinline__ void decode_block(int L, int nqb, int H, int& qb, int& h, int& b) {
  qb = L % nqb;
  h = (L / nqb) % H;
  b = L / (nqb * H);
}

// ---- the two key segments as one run of tiles: T0 = kv_tiles(n[0]) tiles of segment 0, then those of segment 1
__device__ __forceinline__ int kv_tiles(int n) { return (n + KVT - 1) / KVT; }
struct KvTile { int seg, kv0, n; };              // tile t: keys kv0 .. kv0 + 63 of segment seg, which has n keys
__device__ __forceinline__ KvTile kv_tile(const AttnParams& p, int t, int T0) {
  const int seg = (t < T0) ? 0 : 1;
  return {seg, (seg ? (t - T0) : t) * KVT, p.n[seg]};
}

// ---- tail rules of the LDS-DMA kernels (n % 8 == 0).  K: rows beyond n are clamped duplicates of the last valid key (a valid
// score).  V^T: an LDS-DMA instruction moves 8 rows of 128 B, lane -> row row0 + (lane >> 3), LDS slot lane & 7, which holds the
// global 8-key chunk slot ^ ((row >> 1) & 7); whole chunks beyond n come from the zero page, so tail keys add nothing to O.
__device__ __forceinline__ int k_tail_row(int kv0, int row, int n) { return min(kv0 + row, n - 1); }
__device__ __forceinline__ int vt_row(int row0, int lane) { return row0 + (lane >> 3); }
__device__ __forceinline__ int vt_chunk(int row, int lane) { return (lane & 7) ^ ((row >> 1) & 7); }
// per-lane byte offset from the tile's V^T base (full tiles) ...
__device__ __forceinline__ unsigned vt_lane_off(int row0, int lane, int ldv) {
  const int row = vt_row(row0, lane);
  return (unsigned)(row * ldv + vt_chunk(row, lane) * 8) * 2u;
}
// ... and the per-lane source of any tile; base = V^T of the (batch, head) at key kv0
__device__ __forceinline__ const char* vt_chunk_src(const char* base, int row0, int lane, int ldv, int kv0, int n, const unsigned short* zero_page) {
  const int row = vt_row(row0, lane), chunk = vt_chunk(row, lane);
  const bool valid = (kv0 + chunk * 8) < n;
  return valid ? base + ((size_t)row * ldv + chunk * 8) * 2 : reinterpret_cast<const char*>(zero_page + (lane & 7) * 8);
}
// the ones-row group (rows D .. D + 7 of the V^T image): row D = ones in the first nvalid columns, zeros elsewhere
template <int DT, int D>
__device__ __forceinline__ const unsigned short* ones_group_src(int lane, int nvalid, const unsigned short (*ones_page)[8], const unsigned short* zero_page) {
  const int row = vt_row(D, lane), chunk = vt_chunk(row, lane);
  const bool one = (row == D) && (chunk * 8 < nvalid);
  return one ? ones_page[DT == IDF_BF16 ? 0 : 1] : zero_page + (lane & 7) * 8;
}

// ---- epilogue.  o[mt][r] of lane (l31, hi): element e = mt*32 + (r&3) + 8*(r>>2) + 4*hi of query l31.
// Softmax denominator from the all-ones V^T row: row e = d of O^T sits in tile d/32 (the last), register 4*((d%32)/8) of the
// hi = 0 lanes (d % 8 == 0); broadcast from lane l31 to its hi = 1 partner.
__device__ __forceinline__ float denominator_from_ones_row(const f32x16& o_last, int d, int l31) {
  const int sel = (d & 31) >> 3;
  const float lv = sel == 0 ? o_last[0] : (sel == 1 ? o_last[4] : (sel == 2 ? o_last[8] : o_last[12]));
  return __shfl(lv, l31, 64);
}
// the lane's share of its query's row, normalised and packed: 8-B pieces at elements 8 qd + 4 hi of orow (LDS staging or global)
template <int DT, int NMT>
__device__ __forceinline__ void pack_o_rows(const f32x16 (&o)[NMT], float inv, int d, int hi, unsigned short* orow) {
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int e = mt * 32 + 8 * qd + 4 * hi;
      if (e < d) {   // d % 8 == 0 and e % 4 == 0 -> the 4 columns are all valid
        u32x2 pk = {pack2<DT>(o[mt][4 * qd] * inv, o[mt][4 * qd + 1] * inv),
                    pack2<DT>(o[mt][4 * qd + 2] * inv, o[mt][4 * qd + 3] * inv)};
        *reinterpret_cast<u32x2*>(orow + e) = pk;
      }
    }
}
// Coalesced store tail.  A lane owns ONE query row in 8-byte pieces: stored directly that is one 8-B store per piece at a
// 2*ldo-byte lane stride -- store-issue-bound, every piece a partial 32-B sector.  Instead each wave transposes its block through
// its own LDS slice `ow` ([rows][dch * 8], written by pack_o_rows) and writes 16 B per lane with consecutive lanes on consecutive
// chunks of a row.  lds_wave_fence: the wave's own LDS accesses are complete, in order, before what follows.
__device__ __forceinline__ void lds_wave_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
// 16-B chunk c of the block (row-major: byte offset 16 c) -> row q0 + c / dch of the output, when that query exists
__device__ __forceinline__ void store_chunk16(const unsigned short* ow, unsigned short* obase, int ldo, int q0, int nq, int c, int dch) {
  const int row = c / dch, col = c - row * dch;
  const u32x4 v = *reinterpret_cast<const u32x4*>(ow + c * 8);
  if (q0 + row < nq) *reinterpret_cast<u32x4*>(obase + (size_t)(q0 + row) * ldo + col * 8) = v;
}
template <int ROWS, int DCH>
__device__ __forceinline__ void store_block16(const unsigned short* ow, unsigned short* obase, int ldo, int q0, int nq, int lane) {
  static_assert((ROWS * DCH) % 64 == 0, "whole wave store instructions");
  lds_wave_fence();
#pragma unroll
  for (int j = 0; j < ROWS * DCH / 64; ++j) store_chunk16(ow, obase, ldo, q0, nq, lane + 64 * j, DCH);
}

// ================================================================================================================
// Host section
// ================================================================================================================
// What every LDS-DMA launcher needs of a launch (else IDF_ATTN2_UNSUPPORTED and the caller falls back): n % 8 == 0; K / V^T rows,
// bases and batch strides 16-B aligned; O and Q likewise (the LDS-transposed epilogue stores O and the kernels read Q as 16-B
// vectors; the 32-query kernel with its 8-B stores and idf_attention's own ldo % 4 contract takes the others); and, the per-lane
// DMA offsets being 32-bit and signed, a 64-key K tile and the vt_rows V^T rows a kernel fetches of a (batch, head) below 2 GB.
inline bool attn_dma_eligible(const AttnParams& p, int vt_rows) {
  if ((p.n[0] % 8) || (p.n[1] % 8)) return false;
  if ((p.ldk[0] % 8) || (p.ldv[0] % 8) || (p.n[1] > 0 && ((p.ldk[1] % 8) || (p.ldv[1] % 8)))) return false;
  if (!aligned16(p.k[0]) || !aligned16(p.vt[0]) || !aligned16(p.k[1]) || !aligned16(p.vt[1])) return false;
  if ((p.sK[0] % 8) || (p.sV[0] % 8) || (p.sK[1] % 8) || (p.sV[1] % 8)) return false;
  if (!aligned16(p.out) || (p.ldo % 8) || (p.sO % 8) || !aligned16(p.q) || (p.ldq % 8) || (p.sQ % 8)) return false;
  for (int seg = 0; seg < (p.n[1] > 0 ? 2 : 1); ++seg)
    if ((long long)KVT * p.ldk[seg] * 2 >= (1ll << 31) || (long long)vt_rows * p.ldv[seg] * 2 >= (1ll << 31)) return false;
  return true;
}
// a tuning mode's start value: environment variable `name` when it holds 0 .. max, else dflt (it may hold a value of an older
// ABI that named kernels which left the library: out of range = default, the same range idf_set_tuning accepts)
inline int attn_mode_from_env(const char* name, int dflt, int max) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return (v < 0 || v > max) ? dflt : v;
}

}  // namespace idfattn

// 64-queries-per-wave LDS-DMA kernel for d in {24, 40, 56} (attention4.hip): max-free softmax with the reference value
// folded into the K.Q^T MFMA, K fragments read one tile ahead, XCD-aware 1-D grid.  Returns IDF_ATTN2_UNSUPPORTED when the
// shape does not qualify (the caller then runs the 32-queries-per-wave kernel of attention.hip).
// Attention mode (idf_set_tuning(IDF_TUNE_ATTN2), env IDF_ATTN2): 0 = 32-query kernel only; 1 = this kernel when the shape
// qualifies, as two 4-wave workgroups per CU (256 queries each; default); 2 = as ONE 8-wave workgroup per 512 queries (every
// K / V^T tile shared by eight waves: 1.4 LDS-DMA instructions per wave and tile instead of 2.75 -- +1 % in isolation,
// -3 % inside the forward, where the two independent workgroups of a CU overlap better: profiles/r03_attn_ab*_B64.log,
// r03_shape_profile_B64_attn{1,2}.log); 3 = mode 1 with the plain block order (A/B of the XCD mapping); 4 / 5 = attention4w.hip
// (round 6: the asm-scheduled stream, d = 40 only) with 128 queries per wave on one wave per SIMD / 64 on two (default 5).
// The round-1 / round-2 variants this kernel replaced (attention2.hip: classic / lazy / software-pipelined online softmax;
// attention5.hip: 8-wave ping-pong form) were measured slower and live under profiles/archive_rejected_kernels/ with their logs in
// profiles/r02_attn_*.
#define IDF_ATTN2_UNSUPPORTED (-100)
#ifndef IDF_ATTN2_DEFAULT
#define IDF_ATTN2_DEFAULT 5
#endif
#include <atomic>
extern std::atomic<long long> idf_stat_attn2_launches;   // process-global launch counter (idf_get_stat)
extern std::atomic<long long> idf_stat_attn_res_launches;   // launches served by the resident-key (RES) instantiation of attn_kernel
int idf_attn2_mode();
int idf_attn2_set_mode(int v);
int idf_launch_attn4(const idfattn::AttnParams& p, int B, int dtype, hipStream_t s);
// one-wave-per-SIMD form of the d = 40 kernel (attention4w.hip, round 6): 128 queries per wave, asm-scheduled stream
int idf_launch_attn4w(const idfattn::AttnParams& p, int B, int dtype, int variant /* mode 4: 128 queries per wave, 5: 64, 6: 128 + persistent */, hipStream_t s);
// 32-queries-per-wave LDS-DMA kernel for d in {80, 160} (attention8.hip, round 5): K / V^T rings by LDS-DMA, deferred-rescale
// running max, XCD-aware 1-D grid.  Mode (idf_set_tuning(IDF_TUNE_ATTN8), env IDF_ATTN8): 0 = off (attention.hip's register-staged
// kernel); 1 = on (d = 80: two 4-wave workgroups per CU with the K fragments read one tile ahead; d = 160: one 8-wave workgroup
// per 256 queries, 4-wave workgroups below 256 queries); 2 = 8-wave workgroups at d = 80 and at every d = 160 size; 3 = mode 1
// with the plain block order; 4 = d = 160 on 4-wave workgroups; 5 / 6 = d = 80 software-pipelined (K.Q^T of tile t+1 issued in
// front of tile t's exponentials) on 4- / 8-wave workgroups.  Returns IDF_ATTN2_UNSUPPORTED when the shape does not qualify.
#ifndef IDF_ATTN8_DEFAULT
#define IDF_ATTN8_DEFAULT 1
#endif
extern std::atomic<long long> idf_stat_attn8_launches;
int idf_attn8_mode();
int idf_attn8_set_mode(int v);
int idf_launch_attn8(const idfattn::AttnParams& p, int B, int dtype, hipStream_t s);
