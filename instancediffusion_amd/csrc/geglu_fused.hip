// geglu_fused.hip -- the GEGLU projection of a C = 640 transformer block with the activation rows RESIDENT IN REGISTERS (gfx950):
//     out[m][j] = value * gelu(gate),   (value | gate) = LN(x) . W1^T + b1        (attention.py:36-47 GEGLU; K = 640, N = 5120,
// weight rows packed [16 value | 16 gate] per 32, LayerNorm folded: C ABI idf_gemm with IDF_EPI_BIAS | GEGLU | GEGLU_P32 | LN_ROW).
//
// Why.  On the persistent GEMM kernel (gemm_big.hip) this launch runs at 860-875 TF (0.98 ms at 128 rows of 32 x 32 latents): the
// LayerNorm fold + GELU epilogue of a 256 x 320 tile is ~27 % of a K = 640 tile with the matrix pipe idle (both waves of a SIMD are
// in it together).  Here -- the machinery of mlp320w_kernel / qkv320w_kernel (mw_prims.h, a generated `asm volatile` stream,
// tools/gen_gegluw_stream.py -> gegluw_stream.inc):
//   * a workgroup is 4 waves, one per SIMD; wave w owns rows 32 w .. + 31 of a 128-row tile, whose 640 elements per row stay in
//     40 MFMA operand fragments in asm-owned AGPRs (a0..a159) and serve all 5120 packed weight rows;
//   * the weight image streams through a 2-slot LDS ring in 160 chunks of 32 packed rows (= 16 output columns; 40 KB: ten K-tiles
//     of [32 rows][64 k], 128-B rows, 16-B slot ^= (row >> 1) & 7) by LDS-DMA, ten pieces per wave and chunk, one barrier per chunk;
//   * per pipeline step: the 40 MFMAs of chunk i + 1 (two accumulators, even / odd k-steps) carry the epilogue of chunk i in their
//     gaps: sum of the two accumulators, LayerNorm fold + bias, GEGLU in the fused MLP's x sigmoid(p(x)) form, 16-bit, 8 B per lane
//     into a wave-private staging image; every fourth chunk the image (32 rows x 128 B) is stored as whole lines;
//   * counted vmcnt everywhere; the next tile's rows go out in the tile's last step BEFORE its stores.
// Taken by idf_gemm when K = 640, N = 5120, the epilogue is exactly BIAS | GEGLU | GEGLU_P32 | LN_ROW with the statistics handed
// in, M % 128 == 0 and M >= two tiles per CU; everything else stays on gemm_big.hip.  Same arithmetic per output element as the
// persistent kernel up to the order of the K sum (two partial sums) and the fma contraction of the fold.
// LDS: 2 x 40 KB ring + 40 KB (c | d of all 5120 packed rows) + 4 x 4 KB staging = 136 KB.
#include "mw_row.h"

using namespace idfcore;
using namespace idfmw;

namespace {

constexpr int GW_N = 5120;                                                        // 160 chunks of 32 packed rows
using GwRow = Row640<GW_N>;
constexpr int GW_STG_OFF = GwRow::TAIL_OFF, GW_SMEM = GW_STG_OFF + 4 * 4096;
static_assert(GW_SMEM == 136 * 1024, "LDS budget in the header comment");

struct GwParams {
  const unsigned short* x; int ldx;
  const float* ln_stats;                 // [M][2] (mu, rstd)
  const unsigned short* w; int ldw;      // [5120][640] gamma-folded, rows packed [16 value | 16 gate] per 32
  const float* c; const float* d;        // [5120] row sums of w; beta term + bias (packed order)
  unsigned short* out; int ldo;          // [M][>= 2560]
  int M;
};

struct GwCtx {
  unsigned w1a[4];                       // LDS byte addresses of the W fragment reads of the chunk whose MFMAs run (per lane, by ks & 3)
  unsigned cda;                          // c of the chunk in its epilogue (+ 16 hi); d at + 5120 floats
  unsigned qwj[2], qr[4], qst[4];        // staging image: this chunk's two 8-B write addresses, read-back addresses, store offsets
  const void* obase;
  float nmu, rstd, k1, k2, k3, one, lo8, hi8;
  unsigned w1dst, w1_vj; const char* wb;
  const unsigned short* xnext; const float* snext; bool has_next;
};

#ifndef GEGLUW_STREAM_INC
#define GEGLUW_STREAM_INC "gegluw_stream.inc"
#endif
#include GEGLUW_STREAM_INC

template <int DT>
__global__ __launch_bounds__(256, 1) void geglu640w_kernel(const GwParams p, const int tiles) {
  asm volatile("" ::: "a0", "a161");               // the asm-owned AGPR block: x fragments a0..a159, a160:161 the next tile's (mu, rstd)
  extern __shared__ __attribute__((aligned(128))) char smem[];
  GwCtx c;
  c.k1 = 1.0142652e-3f; c.k2 = -1.0677574e-1f; c.k3 = -2.3011213f; c.one = 1.0f; c.lo8 = -8.0f; c.hi8 = 8.0f;
  asm volatile("" : "+v"(c.k1), "+v"(c.k2), "+v"(c.k3), "+v"(c.one), "+v"(c.hi8));
  GwRow k;
  k.init(smem, p.x, p.ldx, p.ln_stats, p.w, p.ldw, c);
  const int wave = k.r.wave, hi = k.r.hi, G = k.G;
  // staging image of the wave (mw_row.h): [32 rows][128 B = the 64 output columns of four chunks]; a lane writes slots 2 jj + q
  const unsigned qwb = mw_stage_image(k.r, k.smem_lds + (unsigned)(GW_STG_OFF + wave * 4096), p.ldo, c.qr, c.qst);

  int tile = mw_first_tile(G);
  if (tile >= tiles) return;
  k.prologue(smem, p.c, p.d, tile, c);

  f32x16 acc[2][2];
  auto set_step = [&](int i) {
    k.set_ring(i, c);
    c.cda = k.cd_lds + (unsigned)((32 * i + 4 * hi) * 4);
    const int jj = i & 3;
#pragma unroll
    for (int q = 0; q < 2; ++q) c.qwj[q] = qwb ^ (unsigned)(16 * (2 * jj + q));
    c.obase = reinterpret_cast<const char*>(p.out) + ((size_t)tile * R640_BM + wave * 32) * p.ldo * 2 + (size_t)(i >> 2) * 128;
  };

  for (;;) {
    k.tile_stats(c);
    const int next = tile + G;
    c.has_next = next < tiles;
    c.xnext = k.row_ptr(c.has_next ? next : tile);
    c.snext = k.st_ptr(c.has_next ? next : tile);

    set_step(-1);
    gw_pro<DT, 0>(acc[1], acc[0], c);                              // MFMAs of chunk 0 -> acc[0]; the pieces of chunk 1
    // groups of four steps share a staging image; VMC of a step = the stores issued behind the pieces it waits for
    set_step(0);
    gw_step<DT, 0>(acc[0], acc[1], c);
    set_step(1);
    gw_step<DT, 0>(acc[1], acc[0], c);
    set_step(2);
    gw_step<DT, 0>(acc[0], acc[1], c);
    set_step(3);
    gw_step_st<DT, 0>(acc[1], acc[0], c);
    for (int i = 4; i < GwRow::NCH - 4; i += 4) {                      // steps 4 .. 155
      set_step(i);
      gw_step<DT, 4>(acc[0], acc[1], c);                           // (behind the four stores of step i - 1)
      set_step(i + 1);
      gw_step<DT, 0>(acc[1], acc[0], c);
      set_step(i + 2);
      gw_step<DT, 0>(acc[0], acc[1], c);
      set_step(i + 3);
      gw_step_st<DT, 0>(acc[1], acc[0], c);
    }
    set_step(GwRow::NCH - 4);
    gw_step<DT, 4>(acc[0], acc[1], c);
    set_step(GwRow::NCH - 3);
    gw_step<DT, 0>(acc[1], acc[0], c);
    set_step(GwRow::NCH - 2);
    gw_step<DT, 0>(acc[0], acc[1], c);
    set_step(GwRow::NCH - 1);
    gw_last<DT, 0>(acc[1], acc[0], c);                             // epilogue of chunk 159 + the store group; the next tile's rows first
    if (!c.has_next) break;
    tile = next;
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");               // rows + statistics landed; the 4 stores behind them may fly
  }
}

MwKnob g_gegluw_knob{"IDF_GEGLU_ROW", 1};

}  // namespace

int idf_gegluw_set_mode(int v) { return g_gegluw_knob.set(v); }

// idf_gemm tries this first for GEGLU launches; IDF_BIG_UNSUPPORTED = the shape / epilogue is not this kernel's
int idf_launch_geglu640w(const idfcore::CoreParams& p, int dtype, hipStream_t s) {
  if (g_gegluw_knob.get() == 0) return IDF_BIG_UNSUPPORTED;
  if (!mw_row_eligible(p, dtype, R640_K, GW_N, R640_BM, GW_N / 2) || p.vt_out) return IDF_BIG_UNSUPPORTED;
  if (p.epi != (IDF_EPI_BIAS | IDF_EPI_GEGLU | IDF_EPI_GEGLU_P32 | IDF_EPI_LN_ROW) || p.stat_parts || p.ln_stats_out) return IDF_BIG_UNSUPPORTED;
  GwParams q;
  q.x = p.A; q.ldx = p.lda; q.ln_stats = p.ln_stats; q.w = p.W; q.ldw = p.ldw; q.c = p.ln_c; q.d = p.bias;
  q.out = static_cast<unsigned short*>(p.out); q.ldo = p.ldo; q.M = p.M;
  return dtype == IDF_BF16 ? mw_row_launch<GwParams, geglu640w_kernel<IDF_BF16>, GW_SMEM, R640_BM>(q, s)
                           : mw_row_launch<GwParams, geglu640w_kernel<IDF_F16>, GW_SMEM, R640_BM>(q, s);
}
