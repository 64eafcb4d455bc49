// proj320_stream.hip -- the N = K = 320 projections of a C = 320 SpatialTransformer (proj_in, attn1.out, f_attn.out, the
// cross-attention query, attn2.out, proj_out; call site engine._st; C ABI: idf_gemm, include/idf.h) as a STREAMING kernel with
// the weights RESIDENT IN REGISTERS (gfx950).
//
// Why.  Each of these launches reads [M][320], sometimes a residual of the same size, and writes [M][320] against a 200 KB weight
// image: about 205 operations per element, a streaming operation.  On the persistent GEMM kernel (gemm_big.hip) K = 320 is five
// K-tiles per 256 x 320 tile, so prologue, accumulator turn-around, residual read and store of EVERY tile are exposed and every
// tile re-stages the whole weight image through LDS-DMA: 0.507 ms at M = 1048576 = 0.49 of the HBM peak.  The row-resident
// skeleton (mw_row.h: rows in registers, weights streaming) is the wrong way round for this shape; here the roles are swapped:
//   * one persistent workgroup per CU, 4 waves, one per SIMD.  Wave w owns output columns 80 w .. + 79 and loads their
//     [80][320] weight rows ONCE per launch into 50 MFMA operand fragments in asm-owned AGPRs a0..a199 (5 column tiles of 16 x
//     10 k-steps of 32);
//   * the activation rows stream in blocks of 32 through a 3-slot LDS ring by LDS-DMA pieces of 8 rows x 128 B (whole lines; the
//     image is the K-tile image of mw_row.h: [5 K-tiles][32 rows][128 B], 16-B slot ^= (row >> 1) & 7), three blocks ahead;
//     all four waves read the same block (2 x 10 ds_read_b128 per lane);
//   * the product runs on v_mfma_f32_16x16x32 with the operands swapped (A = W fragment, B = x fragment), so a lane's four
//     accumulator registers are four CONSECUTIVE columns of one row: 100 MFMAs per wave and block = 1 600 matrix-pipe cycles,
//     against the ~5 250 cycles per block that 0.32 ms per launch allows.  The 32x32x16 form would need the columns split
//     96 / 96 / 64 / 64 (uneven waves, 240 weight registers on two of them) and packs two columns per register pair;
//   * the residual rows arrive by the same pieces in a 4-slot ring; the epilogue reads them there (8 B per lane), applies
//     [LN_ROW] + bias [+ gate x .. + residual] in fp32 exactly as gemm_core.h's epilogue8 does, and writes the 16-bit result back
//     IN PLACE; after a barrier all 256 threads store the block as whole 640-B rows, 8 lanes per 128-B line (a wave's own
//     80-column slice is 160 B per row and not line-aligned);
//   * out_stats: in that store pass 8 lanes hold a whole output row as stored, so (mu, rstd) is the exact two-pass form of
//     idf_row_stats over three shuffles -- final values, no partial slots, no finalize launch;
//   * every load of the loop is an LDS-DMA and every store an `asm volatile`, so the one wait per block is a counted vmcnt:
//     the loads of block i are followed by P store groups and P - 1 load groups (P = 3 blocks ahead).
// A block's rows belong to one workgroup and its residual has landed in LDS before its first store is issued, so out == res
// and out == A are safe.  Rows do not interact: the same row in two blocks gives the same bits.
// Taken by idf_gemm for K = N = 320, batch 1, no vt_out, M % 32 == 0, M >= 2 x 256 x (number of CUs) (the rule of qkv320w_kernel), epilogue BIAS, BIAS | RES,
// BIAS | RES | GATE or BIAS | LN_ROW with the statistics handed in, each with or without out_stats.
// LDS: 3 x 20 KB (x) + 4 x 20 KB (residual / output staging) + 3 x 256 B (LN statistics) = 140.75 KB.
#include "mw_row.h"

using namespace idfcore;
using namespace idfmw;

namespace {

constexpr int PS_BM = 32, PS_C = 320;
constexpr int PS_MIN_ROWS_PER_CU = 512;                  // dispatch threshold: two 256-row tiles per CU, the rule of qkv320w_kernel
constexpr int PS_P = 3;                                  // blocks in flight ahead of the one being computed
constexpr int PS_NX = 3, PS_NR = 4;                      // ring slots: x (refilled behind the block's MFMAs), residual / output
constexpr int PS_SLOT = 5 * 32 * 128;                    // one block: 5 K-tiles x [32 rows][64 k]
constexpr int PS_RO_OFF = PS_NX * PS_SLOT, PS_ST_OFF = PS_RO_OFF + PS_NR * PS_SLOT;
constexpr int PS_SMEM = PS_ST_OFF + PS_NX * 256;
enum { PS_PLAIN = 0, PS_RES = 1, PS_LN = 2 };

struct PsParams {
  const unsigned short* x; int ldx;
  const unsigned short* w; int ldw;      // [320][320] (gamma-folded for LN)
  const float* bias;                     // [320] (LN: beta term + bias)
  const float* c; const float* ln_stats; // LN: row sums of w; [M][2] (mu, rstd)
  const unsigned short* res; int ldr;
  const float* gate;                     // device scalar, or NULL (= 1)
  unsigned short* out; int ldo;
  float* out_stats; float eps;           // [M][2], or NULL
  int M;
};

// one LDS-DMA piece: 64 lanes x 16 B (or 4 B) from sbase + voff to LDS address lds + 16 (4) lane.  m0 is declared clobbered; the
// backend answers that m0 is reserved (it keeps no value there across a statement) with a warning per statement, which build.sh
// switches off for this file (-Wno-inline-asm)
__device__ __forceinline__ void ps_dma16(const void* sbase /* uniform */, unsigned voff, unsigned lds /* uniform */) {
  lds = __builtin_amdgcn_readfirstlane(lds);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds), "v"(voff), "s"(sbase) : "memory", "m0");
}
__device__ __forceinline__ void ps_dma4(const void* sbase /* uniform */, unsigned voff, unsigned lds /* uniform */) {
  lds = __builtin_amdgcn_readfirstlane(lds);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(lds), "v"(voff), "s"(sbase) : "memory", "m0");
}
// weight fragment F (registers a[4 F : 4 F + 3]) <- 16 bytes at byte offset OFF of the lane's weight row pointer
template <int F, int OFF> __device__ __forceinline__ void ps_load_w(const unsigned short* rowp) {
  asm volatile("global_load_dwordx4 a[%c1:%c2], %0, off offset:%c3" ::"v"(rowp), "n"(4 * F), "n"(4 * F + 3), "n"(OFF) : "memory");
}
// acc (+)= W fragment F (A, asm-owned AGPRs) . x fragment (B, VGPRs): D[column 4 (lane >> 4) + r of the tile][row lane & 15]
template <int DT, int F, bool FIRST> __device__ __forceinline__ void ps_mfma(f32x4& acc, const u32x4& x) {
  if constexpr (FIRST) {
    if constexpr (DT == IDF_BF16) asm volatile("v_mfma_f32_16x16x32_bf16 %0, a[%c2:%c3], %1, 0" : "=&v"(acc) : "v"(x), "n"(4 * F), "n"(4 * F + 3));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c2:%c3], %1, 0" : "=&v"(acc) : "v"(x), "n"(4 * F), "n"(4 * F + 3));
  } else {
    if constexpr (DT == IDF_BF16) asm volatile("v_mfma_f32_16x16x32_bf16 %0, a[%c2:%c3], %1, %0" : "+v"(acc) : "v"(x), "n"(4 * F), "n"(4 * F + 3));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, a[%c2:%c3], %1, %0" : "+v"(acc) : "v"(x), "n"(4 * F), "n"(4 * F + 3));
  }
}
template <int OFF> __device__ __forceinline__ void ps_store16(unsigned voff, const u32x4& v, const void* sbase /* uniform */) {
  asm volatile("global_store_dwordx4 %0, %1, %2 offset:%c3" ::"v"(voff), "v"(v), "s"(sbase), "n"(OFF) : "memory");
}
__device__ __forceinline__ void ps_store8(unsigned voff, const f32x2& v, const void* sbase /* uniform */) {
  asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}

template <int DT, int MODE, bool STATS>
__global__ __launch_bounds__(256, 1) void proj320s_kernel(const PsParams p, const int blocks) {
  asm volatile("" ::: "a0", "a199");               // the asm-owned AGPR block (this is where the kernel descriptor learns its size)
  extern __shared__ __attribute__((aligned(128))) char smem[];
  constexpr bool RES = MODE == PS_RES, LN = MODE == PS_LN;
  constexpr int NLOAD = 5 + (RES ? 5 : 0) + (LN ? 1 : 0), NSTORE = 5 + (STATS ? 1 : 0);
  constexpr int VMC = PS_P * NSTORE + (PS_P - 1) * NLOAD;   // what was issued behind the loads of the block about to be read
  static_assert(VMC < 64, "vmcnt is a 6-bit counter");
  const RowLane rl = mw_row_lane();
  const int tid = rl.tid, lane = rl.lane, wave = rl.wave, l15 = lane & 15, q = lane >> 4;
  const int G = gridDim.x;
  const unsigned smem_lds = lds_u32(smem);

  const int blk0 = mw_first_tile(G);
  if (blk0 >= blocks) return;
  const int nblk = (blocks - blk0 + G - 1) / G;    // this workgroup's blocks: blk0 + i G

  // epilogue constants of the lane's 5 x 4 columns 80 wave + 16 nt + 4 q + r
  f32x4 bias[5], cc[5];
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    bias[nt] = *reinterpret_cast<const f32x4*>(p.bias + 80 * wave + 16 * nt + 4 * q);
    if constexpr (LN) cc[nt] = *reinterpret_cast<const f32x4*>(p.c + 80 * wave + 16 * nt + 4 * q);
  }
  float gm = 1.0f;
  if constexpr (RES) if (p.gate) gm = p.gate[0];
  // the compiler must wait for these loads HERE: left pending on its scoreboard, its own vmcnt(0) in front of their first use
  // inside the loop would drain the stream in every block
#pragma unroll
  for (int nt = 0; nt < 5; ++nt) {
    asm volatile("" : "+v"(bias[nt]));
    if constexpr (LN) asm volatile("" : "+v"(cc[nt]));
  }
  asm volatile("" : "+v"(gm));

  // LDS-DMA role (mw_row.h): piece kt = rows 8 wave .. + 7 of K-tile kt; lane -> row 8 wave + lane / 8, 16-B slot lane % 8
  const int prow = 8 * wave + (lane >> 3);
  const unsigned pswz = (unsigned)((((lane & 7) ^ ((prow >> 1) & 7)) << 4));
  const unsigned x_voff = (unsigned)(prow * p.ldx * 2) + pswz;
  const unsigned r_voff = RES ? (unsigned)(prow * p.ldr * 2) + pswz : 0u;
  auto issue = [&](int i) {                        // the loads of block i (behind the last block: the last block again, unused --
    const int ii = i < nblk ? i : nblk - 1;        // at most 3 of a workgroup's >= 16 blocks; it keeps the counted wait uniform)
    const size_t m0 = (size_t)(blk0 + ii * G) * PS_BM;
    const char* xb = reinterpret_cast<const char*>(p.x) + m0 * p.ldx * 2;
    const unsigned xs = smem_lds + (unsigned)((i % PS_NX) * PS_SLOT + wave * 1024);
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) ps_dma16(xb + kt * 128, x_voff, xs + (unsigned)(kt * 4096));
    if constexpr (RES) {
      const char* rb = reinterpret_cast<const char*>(p.res) + m0 * p.ldr * 2;
      const unsigned rs = smem_lds + (unsigned)(PS_RO_OFF + (i % PS_NR) * PS_SLOT + wave * 1024);
#pragma unroll
      for (int kt = 0; kt < 5; ++kt) ps_dma16(rb + kt * 128, r_voff, rs + (unsigned)(kt * 4096));
    }
    if constexpr (LN)                              // (every wave brings the block's 32 (mu, rstd) pairs: equal counts, equal bytes)
      ps_dma4(reinterpret_cast<const char*>(p.ln_stats + 2 * m0), (unsigned)(lane * 4), smem_lds + (unsigned)(PS_ST_OFF + (i % PS_NX) * 256));
  };

  // kernel prologue: the first P blocks, then the wave's weight fragments
#pragma unroll
  for (int i = 0; i < PS_P; ++i) issue(i);
  {
    const unsigned short* wp = p.w + (size_t)(80 * wave + l15) * p.ldw + 8 * q;
    mw_static_for<5>([&](auto nt) {
      const unsigned short* wr = wp + (size_t)(16 * decltype(nt)::value) * p.ldw;
      mw_static_for<10>([&](auto ks) { ps_load_w<decltype(nt)::value * 10 + decltype(ks)::value, 64 * decltype(ks)::value>(wr); });
    });
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // per-lane LDS offsets inside a slot.  x fragment of rows 16 mt + l15, k-step ks: K-tile ks / 2, slot 4 (ks & 1) + q
  unsigned xoff[2][2], eoff[2][5];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int row = 16 * mt + l15, sw = (row >> 1) & 7;
#pragma unroll
    for (int h = 0; h < 2; ++h) xoff[mt][h] = (unsigned)(row * 128 + (((4 * h + q) ^ sw) << 4));
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {               // the lane's four columns of tile nt: 8 B of the residual / output image
      const int n = 80 * wave + 16 * nt + 4 * q;
      eoff[mt][nt] = (unsigned)((n >> 6) * 4096 + row * 128 + ((((n & 63) >> 3) ^ sw) << 4) + (n & 7) * 2);
    }
  }
  // store pass: thread -> row tid / 8, 16-B slot tid % 8 of every K-tile
  const int crow = tid >> 3, cj = tid & 7;
  const unsigned coff = (unsigned)(crow * 128 + ((cj ^ ((crow >> 1) & 7)) << 4));
  const unsigned o_voff = (unsigned)(crow * p.ldo * 2 + cj * 16);

  for (int i = 0; i < nblk; ++i) {
    // this block's pieces of this wave have landed; behind the barrier everybody's have
    asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"n"(VMC) : "memory");
    const char* xs = smem + (i % PS_NX) * PS_SLOT;
    char* ro = smem + PS_RO_OFF + (i % PS_NR) * PS_SLOT;
    const size_t m0 = (size_t)(blk0 + i * G) * PS_BM;

    u32x4 xf[2][10];
#pragma unroll
    for (int ks = 0; ks < 10; ++ks)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) xf[mt][ks] = *reinterpret_cast<const u32x4*>(xs + xoff[mt][ks & 1] + (ks >> 1) * 4096);
    f32x4 acc[2][5];
    mw_static_for<10>([&](auto ks) {
      mw_static_for<5>([&](auto nt) {
        constexpr int KS = decltype(ks)::value, NT = decltype(nt)::value;
        ps_mfma<DT, NT * 10 + KS, KS == 0>(acc[0][NT], xf[0][KS]);
        ps_mfma<DT, NT * 10 + KS, KS == 0>(acc[1][NT], xf[1][KS]);
      });
    });
    // MFMA -> VALU wait states (the compiler does not see into the statements above); the operands tie the readers to it
    asm volatile("s_nop 15\n\ts_nop 15"
                 : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[0][4]), "+v"(acc[1][0]), "+v"(acc[1][1]),
                   "+v"(acc[1][2]), "+v"(acc[1][3]), "+v"(acc[1][4]));

    // epilogue (gemm_core.h epilogue8's arithmetic): [rstd (acc - mu c)] + bias, [res + gate x ..], 16 bit, into the image
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x2 st = {0.0f, 1.0f};
      if constexpr (LN) st = *reinterpret_cast<const f32x2*>(smem + PS_ST_OFF + (i % PS_NX) * 256 + (16 * mt + l15) * 8);
#pragma unroll
      for (int nt = 0; nt < 5; ++nt) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[mt][nt][r];
          if constexpr (LN) v[r] = st[1] * fmaf(-st[0], cc[nt][r], v[r]);
          v[r] += bias[nt][r];
        }
        if constexpr (RES) {
          const u32x2 rr = *reinterpret_cast<const u32x2*>(ro + eoff[mt][nt]);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            v[2 * h] = fmaf(gm, v[2 * h], Elem<DT>::to_f32((unsigned short)(rr[h] & 0xffffu)));
            v[2 * h + 1] = fmaf(gm, v[2 * h + 1], Elem<DT>::to_f32((unsigned short)(rr[h] >> 16)));
          }
        }
        *reinterpret_cast<u32x2*>(ro + eoff[mt][nt]) = u32x2{pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3])};
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    issue(i + PS_P);                               // x slot of this block, residual slot of the block before: both read out

    // store pass: whole rows, 8 lanes per 128-B line
    u32x4 o[5];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) o[kt] = *reinterpret_cast<const u32x4*>(ro + coff + kt * 4096);
    const char* ob = reinterpret_cast<const char*>(p.out) + m0 * p.ldo * 2;
    ps_store16<0>(o_voff, o[0], ob);
    ps_store16<128>(o_voff, o[1], ob);
    ps_store16<256>(o_voff, o[2], ob);
    ps_store16<384>(o_voff, o[3], ob);
    ps_store16<512>(o_voff, o[4], ob);
    if constexpr (STATS) {                         // (mu, rstd) of the row as stored: exact two-pass over the row's 8 lanes
      float f[40];
#pragma unroll
      for (int kt = 0; kt < 5; ++kt) unpack8<DT>(o[kt], f + 8 * kt);
      float sum = 0.0f;
#pragma unroll
      for (int e = 0; e < 40; ++e) sum += f[e];
      sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64); sum += __shfl_xor(sum, 4, 64);
      const float mean = sum * (1.0f / PS_C);
      float m2 = 0.0f;
#pragma unroll
      for (int e = 0; e < 40; ++e) { const float d = f[e] - mean; m2 = fmaf(d, d, m2); }
      m2 += __shfl_xor(m2, 1, 64); m2 += __shfl_xor(m2, 2, 64); m2 += __shfl_xor(m2, 4, 64);
      const f32x2 mr = {mean, rsqrtf(m2 * (1.0f / PS_C) + p.eps)};
      if (cj == 0) ps_store8((unsigned)(crow * 8), mr, reinterpret_cast<const char*>(p.out_stats + 2 * m0));
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int DT>
int ps_launch(const PsParams& q, int mode, hipStream_t s) {
  const bool st = q.out_stats != nullptr;
  if (mode == PS_PLAIN) return st ? mw_row_launch<PsParams, proj320s_kernel<DT, PS_PLAIN, true>, PS_SMEM, PS_BM>(q, s)
                                  : mw_row_launch<PsParams, proj320s_kernel<DT, PS_PLAIN, false>, PS_SMEM, PS_BM>(q, s);
  if (mode == PS_RES) return st ? mw_row_launch<PsParams, proj320s_kernel<DT, PS_RES, true>, PS_SMEM, PS_BM>(q, s)
                                : mw_row_launch<PsParams, proj320s_kernel<DT, PS_RES, false>, PS_SMEM, PS_BM>(q, s);
  return st ? mw_row_launch<PsParams, proj320s_kernel<DT, PS_LN, true>, PS_SMEM, PS_BM>(q, s)
            : mw_row_launch<PsParams, proj320s_kernel<DT, PS_LN, false>, PS_SMEM, PS_BM>(q, s);
}

}  // namespace

MwKnob idf_proj_row_knob{"IDF_PROJ_ROW", 1};
int idf_projw_set_mode(int v) { return idf_proj_row_knob.set(v); }
// least M the kernel takes on the current device (16 blocks per CU: below, the weight prologue -- 200 KB per CU -- and the
// pipeline fill are not amortised, and the 2-18-row forwards stay on the persistent kernel); 0 = the knob is off
// (IDF_PROJ_MIN_ROWS_PER_CU, a multiple of 64 from 64 up, moves the threshold for A/B runs: profiles/proj320_stream.md)
int idf_projw_min_rows() {
  static int per_cu = 0;
  if (per_cu == 0) {
    const char* e = getenv("IDF_PROJ_MIN_ROWS_PER_CU");
    const int v = e ? atoi(e) : PS_MIN_ROWS_PER_CU;
    per_cu = (v < 2 * PS_BM || v % (2 * PS_BM)) ? PS_MIN_ROWS_PER_CU : v;
  }
  return idf_proj_row_knob.get() ? per_cu * idf_num_cu() : 0;
}

// idf_gemm's plain branch tries this first; IDF_BIG_UNSUPPORTED = the shape / epilogue is not this kernel's (nothing launched)
int idf_launch_proj320s(const idfcore::CoreParams& p, int dtype, float* out_stats, float out_stats_eps, hipStream_t s) {
  if (idf_proj_row_knob.get() == 0) return IDF_BIG_UNSUPPORTED;
  if (p.K != PS_C || p.N != PS_C || !p.out || p.vt_out) return IDF_BIG_UNSUPPORTED;
  if ((p.M % PS_BM) || p.M < idf_projw_min_rows()) return IDF_BIG_UNSUPPORTED;
  if (dtype != IDF_BF16 && dtype != IDF_F16) return IDF_BIG_UNSUPPORTED;
  int mode;
  if (p.epi == IDF_EPI_BIAS) mode = PS_PLAIN;
  else if (p.epi == (IDF_EPI_BIAS | IDF_EPI_RES) || p.epi == (IDF_EPI_BIAS | IDF_EPI_RES | IDF_EPI_GATE)) mode = PS_RES;
  else if (p.epi == (IDF_EPI_BIAS | IDF_EPI_LN_ROW)) mode = PS_LN;
  else return IDF_BIG_UNSUPPORTED;
  if (!p.bias || !aligned16(p.bias)) return IDF_BIG_UNSUPPORTED;
  if (mode == PS_LN && (!p.ln_stats || p.stride_ln_stats || !p.ln_c || !aligned16(p.ln_c) || (((uintptr_t)p.ln_stats) & 7u))) return IDF_BIG_UNSUPPORTED;
  if (mode == PS_RES && (!p.res || !aligned16(p.res) || p.ldr < PS_C || (p.ldr % 8))) return IDF_BIG_UNSUPPORTED;
  if ((p.epi & IDF_EPI_GATE) && !p.gate) return IDF_BIG_UNSUPPORTED;
  if (p.lda < PS_C || p.ldw < PS_C || p.ldo < PS_C || (p.lda % 8) || (p.ldw % 8) || (p.ldo % 8)) return IDF_BIG_UNSUPPORTED;
  if (!aligned16(p.A) || !aligned16(p.W) || !aligned16(p.out)) return IDF_BIG_UNSUPPORTED;
  if (out_stats && (((uintptr_t)out_stats) & 7u)) return IDF_BIG_UNSUPPORTED;
  // 32-bit per-lane offsets inside the weight image and inside a block's rows
  const long long ldmax = p.lda > p.ldo ? (p.lda > p.ldr ? p.lda : p.ldr) : (p.ldo > p.ldr ? p.ldo : p.ldr);
  if ((long long)PS_C * p.ldw * 2 >= (1ll << 31) || (long long)PS_BM * ldmax * 2 >= (1ll << 31)) return IDF_BIG_UNSUPPORTED;
  // in place is fine row for row (a block's operands are in LDS before its first store); a shifted overlap is not this kernel's
  if (p.out == (const void*)p.A && p.ldo != p.lda) return IDF_BIG_UNSUPPORTED;
  if (mode == PS_RES && p.out == (const void*)p.res && p.ldo != p.ldr) return IDF_BIG_UNSUPPORTED;
  PsParams q;
  q.x = p.A; q.ldx = p.lda; q.w = p.W; q.ldw = p.ldw; q.bias = p.bias; q.c = p.ln_c; q.ln_stats = p.ln_stats;
  q.res = p.res; q.ldr = p.ldr; q.gate = (p.epi & IDF_EPI_GATE) ? p.gate : nullptr;
  q.out = static_cast<unsigned short*>(p.out); q.ldo = p.ldo; q.out_stats = out_stats; q.eps = out_stats_eps; q.M = p.M;
  return dtype == IDF_BF16 ? ps_launch<IDF_BF16>(q, mode, s) : ps_launch<IDF_F16>(q, mode, s);
}
