// mw_row.h -- the skeleton shared by the row-resident kernels (mlp_fused.hip mlp320w_kernel, qkv_fused.hip qkv320w_kernel,
// qkv640_fused.hip qkv640w_kernel, geglu_fused.hip geglu640w_kernel): 4 waves, one per SIMD; wave w owns 32-row groups of a tile
// whose elements stay in MFMA operand fragments in asm-owned AGPRs; the weight image streams through a 2-slot LDS ring by
// LDS-DMA in chunks of [rows][64 k] K-tiles (128-B rows, 16-B slot ^= (row >> 1) & 7); a generated `asm volatile` stream
// (tools/mw_streamgen.py, primitives mw_prims.h) runs one pipeline step.  Device side: the lane roles, the per-lane addresses
// of that image and of the [32 rows][128 B] staging image, and (Row640) everything the two K = 640 kernels do outside their
// streams and epilogue addresses.  Host side: the launcher, the eligibility checks the idf_launch_* guards share, the mode knob.
// The streams' counted waits are valid only for the instruction sequence emitted around them: after an edit here,
//     python tools/check_attn4w_isa.py --compare OLD_TREE NEW_TREE
#pragma once
#include "gemm_core.h"
#include "mw_prims.h"
#include <atomic>
#include <cstdlib>

namespace idfmw {

struct RowLane { int tid, lane, wave, l31, hi; };
__device__ __forceinline__ RowLane mw_row_lane() {
  RowLane r;
  r.tid = threadIdx.x;
  r.lane = r.tid & 63; r.wave = __builtin_amdgcn_readfirstlane(r.tid >> 6);
  r.l31 = r.lane & 31; r.hi = r.lane >> 5;
  return r;
}
// first tile of a persistent workgroup, XCD-aware: the workgroups of one XCD (blockIdx % 8) walk neighbouring tiles
__device__ __forceinline__ int mw_first_tile(int G) {
  return ((G & 7) == 0) ? (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
}
// LDS-DMA role of a lane in a piece = 8 rows of a K-tile: lane -> row 8 wave + lane / 8, 16-B slot lane % 8; its source byte offset
__device__ __forceinline__ unsigned mw_w1_voff(const RowLane& r, int ldw) {
  const int row = 8 * r.wave + (r.lane >> 3);
  return (unsigned)(row * ldw + (((r.lane & 7) ^ ((row >> 1) & 7)) << 3)) * 2u;
}
// fragment reads of W row l31 of a K-tile image: k-step ks reads 16-B slot (2 (ks & 3) + hi) ^ sw1
__device__ __forceinline__ int mw_sw1(const RowLane& r) { return (r.l31 >> 1) & 7; }
__device__ __forceinline__ void mw_w1_frag(const RowLane& r, unsigned smem_lds, unsigned (&w1o)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) w1o[i] = smem_lds + (unsigned)(r.l31 * 128 + (((2 * i + r.hi) ^ mw_sw1(r)) << 4));
}
// staging image of a wave at LDS address stg: [32 rows][128 B], 16-B slot ^= (row >> 1) & 7.  A lane writes 8 B (+ 8 hi inside
// the slot) of slot s of its row l31 at (the returned base) ^ 16 s, reads back rows lane / 8 + 8 i, slot lane % 8 (qr) and stores
// them at byte offset qst of a [..][ldo] 16-bit matrix: a store instruction writes 8 whole 128-B lines
__device__ __forceinline__ unsigned mw_stage_image(const RowLane& r, unsigned stg, int ldo, unsigned (&qr)[4], unsigned (&qst)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (r.lane >> 3) + 8 * i;
    qr[i] = stg + (unsigned)(row * 128 + (((r.lane & 7) ^ ((row >> 1) & 7)) << 4));
    qst[i] = (unsigned)(row * ldo * 2 + (r.lane & 7) * 16);
  }
  return stg + (unsigned)(r.l31 * 128 + 8 * r.hi + (mw_sw1(r) << 4));
}

// ---- the two K = 640 kernels: a 128-row tile, wave w owns rows 32 w .. + 31 as 40 x fragments a0..a159 (a160:161 = the next
// tile's (mu, rstd)); the [N][640] weight image in N / 32 chunks of 32 rows (40 KB: ten K-tiles) through the 2-slot ring; behind
// the ring the c | d tables of all N rows, then the kernel's own LDS tail.  Ctx = the struct the kernel's streams name; the
// fields used here: w1a[4], w1_vj, w1dst, wb, nmu, rstd.
constexpr int R640_BM = 128, R640_K = 640;
constexpr int R640_SLOT = 10 * 32 * 128;                    // one W chunk: 10 K-tiles x [32 rows][64 k]
constexpr int R640_CD_OFF = 2 * R640_SLOT;                  // c[N] | d[N] fp32

template <int N>
struct Row640 {
  static constexpr int NCH = N / 32, TAIL_OFF = R640_CD_OFF + 2 * N * 4;
  RowLane r;
  int G;
  unsigned smem_lds, cd_lds, w1_voff, w_chunk, w1o[4];
  const unsigned short* x; int ldx; const float* ln_stats;

  template <class Ctx>
  __device__ __forceinline__ void init(char* smem, const unsigned short* x_, int ldx_, const float* st, const unsigned short* w, int ldw, Ctx& c) {
    r = mw_row_lane();
    G = gridDim.x;
    smem_lds = lds_u32(smem);
    x = x_; ldx = ldx_; ln_stats = st;
    w1_voff = mw_w1_voff(r, ldw);
    c.wb = reinterpret_cast<const char*>(w);
    w_chunk = (unsigned)(32 * ldw * 2);
    mw_w1_frag(r, smem_lds, w1o);
    cd_lds = smem_lds + (unsigned)R640_CD_OFF;
  }
  __device__ __forceinline__ const unsigned short* row_ptr(int t) const { return x + (size_t)(t * R640_BM + r.wave * 32 + r.l31) * ldx + 8 * r.hi; }
  __device__ __forceinline__ const float* st_ptr(int t) const { return ln_stats + 2 * (size_t)(t * R640_BM + r.wave * 32 + r.l31); }
  // kernel prologue: c | d of all N rows into LDS, W chunk 0 into ring slot 0, the first tile's rows and statistics
  template <class Ctx>
  __device__ __forceinline__ void prologue(char* smem, const float* cc, const float* dd, int tile, const Ctx& c) const {
    for (int i = r.tid; i < N / 4; i += 256) {
      reinterpret_cast<f32x4*>(smem + R640_CD_OFF)[i] = reinterpret_cast<const f32x4*>(cc)[i];
      reinterpret_cast<f32x4*>(smem + R640_CD_OFF + N * 4)[i] = reinterpret_cast<const f32x4*>(dd)[i];
    }
#pragma unroll
    for (int kt = 0; kt < 10; ++kt) dma16_sv(c.wb + kt * 128, w1_voff, smem_lds + (unsigned)(r.wave * 1024 + kt * 4096));
    {
      const unsigned short* xr = row_ptr(tile);
      mw_static_for<40>([&](auto kc) { mw_load_x2<decltype(kc)::value, decltype(kc)::value>(xr); });
      const float* sp = st_ptr(tile);
      asm volatile("global_load_dwordx2 a[160:161], %0, off" ::"v"(sp) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  // step i of a tile: epilogue of chunk i; MFMAs of chunk i + 1 [ring slot (i + 1) & 1: NCH is even, the parity carries over
  // from tile to tile]; its LDS-DMA pieces bring chunk i + 2 [slot i & 1]
  template <class Ctx>
  __device__ __forceinline__ void set_ring(int i, Ctx& c) const {
    static_assert(NCH % 2 == 0, "the ring slot parity must carry over from tile to tile");
    const unsigned sn = (unsigned)(((i + 1) & 1) * R640_SLOT), sj = (unsigned)((i & 1) * R640_SLOT);
#pragma unroll
    for (int k = 0; k < 4; ++k) c.w1a[k] = w1o[k] + sn;
    int j2 = i + 2;
    if (j2 >= NCH) j2 -= NCH;
    c.w1_vj = w1_voff + (unsigned)j2 * w_chunk;
    c.w1dst = smem_lds + sj + (unsigned)(r.wave * 1024);
  }
  // head of the tile loop: the tile's (mu, rstd) out of a160:161 into c.nmu / c.rstd; returns (mu, rstd)
  template <class Ctx>
  __device__ __forceinline__ f32x2 tile_stats(Ctx& c) const {
    const float mu = __uint_as_float(mw_agpr_read<160>()), rs = __uint_as_float(mw_agpr_read<161>());
    c.nmu = -mu; c.rstd = rs;
    asm volatile("" : "+v"(c.nmu), "+v"(c.rstd));
    return f32x2{mu, rs};
  }
};

}  // namespace idfmw

// ---- host side
// One launch of a persistent row kernel: LDS opt-in (once per device), grid = min(tiles, CUs)
template <class P, void (*KERN)(const P, const int), int SMEM, int BM, int THREADS = 256>
int mw_row_launch(const P& p, hipStream_t s) {
  static std::atomic<unsigned long long> attr_done{0};
  if (const int e = idf_lds_optin(reinterpret_cast<const void*>(KERN), SMEM, attr_done)) return e;
  const int cus = idf_num_cu();
  const int tiles = p.M / BM;
  const int grid = tiles < cus ? tiles : cus;
  hipLaunchKernelGGL(KERN, dim3(grid), dim3(THREADS), SMEM, s, p, tiles);
  return idf_launch_status();
}

// What every idf_launch_* guard of a row kernel asks of an idf_gemm call, for its K, N (weight rows), BM (tile rows) and the
// columns it writes to `out`: 16-bit [M][K] . [N][K]^T, whole tiles and at least two per CU, LayerNorm folded with the
// statistics handed in and the beta term + bias in `bias`, 16-B rows, 32-bit per-lane offsets (the W image, a tile's rows of out).
// The exact epilogue mask and the V^T / by-product arguments stay with the caller.
inline bool mw_row_eligible(const idfcore::CoreParams& p, int dtype, int K, int N, int BM, int out_cols) {
  if (p.K != K || p.N != N || !p.out) return false;
  if ((p.M % BM) || p.M < BM * 2 * idf_num_cu()) return false;
  if (!p.ln_stats || p.stride_ln_stats || !p.ln_c || !p.bias) return false;
  if (dtype != IDF_BF16 && dtype != IDF_F16) return false;
  if (p.lda < K || p.ldw < K || p.ldo < out_cols || (p.lda % 8) || (p.ldw % 8) || (p.ldo % 8)) return false;
  if (!aligned16(p.A) || !aligned16(p.W) || !aligned16(p.out) || !aligned16(p.ln_c) || !aligned16(p.bias)) return false;
  if ((long long)N * p.ldw * 2 >= (1ll << 31) || (long long)BM * p.ldo * 2 >= (1ll << 31)) return false;
  return true;
}
// ... and of its V^T output (the q | k | v kernels): 32-bit offsets inside 32 channel rows
inline bool mw_row_vt_eligible(const idfcore::CoreParams& p) {
  return p.vt_out && aligned16(p.vt_out) && p.ld_vt >= p.M && (p.ld_vt % 8) == 0 && (long long)32 * p.ld_vt * 2 < (1ll << 31);
}

// A mode knob backed by an environment variable that is read once, lazily: '0' = off, anything else = on
struct MwKnob {
  const char* env; int dflt; int v = -1;
  int get() {
    if (v < 0) { const char* e = getenv(env); v = e ? (e[0] == '0' ? 0 : 1) : dflt; }
    return v;
  }
  int set(int nv) { const int prev = get(); v = nv; return prev; }     // idf_set_tuning: returns the previous mode
};
extern MwKnob idf_qkv_row_knob;       // IDF_QKV_ROW: one state for qkv320w_kernel and qkv640w_kernel (defined in qkv_fused.hip)
