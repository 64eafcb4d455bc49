// qkv640_fused.hip -- the fused q | k | v projection of a C = 640 transformer block with the activation rows RESIDENT IN REGISTERS
// (gfx950): out[m][0 .. 1279] = LN(x) . [Wq; Wk]^T, vt[c][m] = (LN(x) . Wv^T)^T   (attention.py:168-172; C ABI idf_gemm with vt_out).
// The K = 640 skeleton shared with geglu640w_kernel (mw_row.h Row640: 4 waves x 32 rows, 40 x fragments in asm-owned AGPRs, the
// [1920][640] weight image through a 2-slot LDS ring in 60 chunks of 32 rows, 40 MFMAs per chunk on two accumulators, one barrier
// per chunk, counted vmcnt) with the epilogues of qkv320w_kernel (qkv_fused.hip): q | k chunks -- fold + bias, 16-bit, 8 B per lane into a staging
// image [32 tokens][128 B] of two chunks, stored as whole lines; V chunks with the MFMA operands swapped -- a lane owns a channel
// and the wave's 32 tokens -- staged [32 channels][64 B], 2 stores per chunk.  Stream: tools/gen_qkv640w_stream.py.
// Taken by idf_gemm when K = 640, N = 1920, vt_col0 = 1280, M % 128 == 0, M >= two tiles per CU, LN_ROW with the statistics
// handed in and BIAS (on the persistent kernel: 843 TF at 128 rows of 32 x 32 latents).
// LDS: 2 x 40 KB ring + 15 KB (c | d) + 1 KB (the waves' (-mu, rstd) tables) + 4 x 4 KB staging = 112 KB.
#include "mw_row.h"

using namespace idfcore;
using namespace idfmw;

namespace {

constexpr int QM_N = 1920, QM_VCH0 = 40;                                          // 60 chunks of 32 rows; chunks 40 .. 59 are V columns
using QmRow = Row640<QM_N>;
constexpr int QM_ST_OFF = QmRow::TAIL_OFF, QM_STG_OFF = QM_ST_OFF + 4 * 256, QM_SMEM = QM_STG_OFF + 4 * 4096;
static_assert(QM_SMEM == 112 * 1024, "LDS budget in the header comment");

struct QmParams {
  const unsigned short* x; int ldx;
  const float* ln_stats;                 // [M][2] (mu, rstd)
  const unsigned short* w; int ldw;      // [1920][640] gamma-folded
  const float* c; const float* d;        // [1920] row sums of w; beta term + bias
  unsigned short* out; int ldo;          // [M][>= 1280]
  unsigned short* vt; int ld_vt;         // [640][>= M]
  int M;
};

struct QmCtx {
  unsigned w1a[4];                       // LDS byte addresses of the W fragment reads of the chunk whose MFMAs run (per lane, by ks & 3)
  unsigned cdq, cdv, stt;                // c of the chunk in its epilogue (q | k: + 16 hi; V: + 4 l31), d at + 1920 floats; the wave's (-mu, rstd) table + 32 hi
  unsigned qwj[4], qr[4], qst[4];        // q | k staging image: this chunk's four 8-B write addresses, read-back addresses, store offsets
  unsigned vw[2], vr[2], vst[2];         // V^T staging image / store offsets
  const void* obase; const void* vtb;
  float nmu, rstd;
  unsigned w1dst, w1_vj; const char* wb;
  const unsigned short* xnext; const float* snext; bool has_next;
};

#ifndef QKV640W_STREAM_INC
#define QKV640W_STREAM_INC "qkv640w_stream.inc"
#endif
#include QKV640W_STREAM_INC

template <int DT>
__global__ __launch_bounds__(256, 1) void qkv640w_kernel(const QmParams p, const int tiles) {
  asm volatile("" ::: "a0", "a161");               // the asm-owned AGPR block: x fragments a0..a159, a160:161 the next tile's (mu, rstd)
  extern __shared__ __attribute__((aligned(128))) char smem[];
  QmCtx c;
  QmRow k;
  k.init(smem, p.x, p.ldx, p.ln_stats, p.w, p.ldw, c);
  const int lane = k.r.lane, wave = k.r.wave, l31 = k.r.l31, hi = k.r.hi, G = k.G;
  // staging slot of the wave (4 KB).  q | k image (mw_row.h): [32 tokens][128 B = the 64 columns of two chunks]; a lane writes
  // slots 4 jj + q.  V^T image (2 KB): [32 channels][64 B], slot ^= (row >> 2) & 3; a lane writes slots 2 hi, 2 hi + 1 of its
  // channel row, reads back rows lane / 4 + 16 i, slot lane % 4.
  const unsigned stg = k.smem_lds + (unsigned)(QM_STG_OFF + wave * 4096);
  const unsigned qwb = mw_stage_image(k.r, stg, p.ldo, c.qr, c.qst);
#pragma unroll
  for (int s = 0; s < 2; ++s) c.vw[s] = stg + (unsigned)(l31 * 64 + (((2 * hi + s) ^ ((l31 >> 2) & 3)) << 4));
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (lane >> 2) + 16 * i;
    c.vr[i] = stg + (unsigned)(row * 64 + (((lane & 3) ^ ((row >> 2) & 3)) << 4));
    c.vst[i] = (unsigned)(row * p.ld_vt * 2 + (lane & 3) * 16);
  }
  c.stt = k.smem_lds + (unsigned)(QM_ST_OFF + wave * 256 + 32 * hi);

  int tile = mw_first_tile(G);
  if (tile >= tiles) return;
  k.prologue(smem, p.c, p.d, tile, c);

  f32x16 acc[2][2];
  auto set_step = [&](int i) {
    k.set_ring(i, c);
    c.cdq = k.cd_lds + (unsigned)((32 * i + 4 * hi) * 4);
    c.cdv = k.cd_lds + (unsigned)((32 * i + l31) * 4);
    const int jj = i & 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) c.qwj[q] = qwb ^ (unsigned)(16 * (4 * jj + q));
    const size_t m0 = (size_t)tile * R640_BM + wave * 32;
    c.obase = reinterpret_cast<const char*>(p.out) + m0 * p.ldo * 2 + (size_t)(i >> 1) * 128;
    c.vtb = reinterpret_cast<const char*>(p.vt) + ((size_t)(32 * (i - QM_VCH0)) * p.ld_vt + m0) * 2;
  };

  for (;;) {
    {
      const f32x2 st = k.tile_stats(c);
      // the wave's table for the V chunks: token t -> (-mu, rstd) at 8 t (both half-waves hold the token; one writes)
      if (hi == 0) *reinterpret_cast<f32x2*>(smem + QM_ST_OFF + wave * 256 + 8 * l31) = f32x2{-st[0], st[1]};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    const int next = tile + G;
    c.has_next = next < tiles;
    c.xnext = k.row_ptr(c.has_next ? next : tile);
    c.snext = k.st_ptr(c.has_next ? next : tile);

    set_step(-1);
    qm_pro<DT, 0>(acc[1], acc[0], c);                              // MFMAs of chunk 0 -> acc[0]; the pieces of chunk 1
    // VMC of a step = the stores the step before issued behind its pieces: 4 after a q | k store step, 2 after a V step
    set_step(0);
    qm_qq<DT, 0>(acc[0], acc[1], c);
    set_step(1);
    qm_qq_st<DT, 0>(acc[1], acc[0], c);
    for (int i = 2; i < QM_VCH0 - 2; i += 2) {                     // steps 2 .. 37
      set_step(i);
      qm_qq<DT, 4>(acc[0], acc[1], c);
      set_step(i + 1);
      qm_qq_st<DT, 0>(acc[1], acc[0], c);
    }
    set_step(QM_VCH0 - 2);
    qm_qq<DT, 4>(acc[0], acc[1], c);
    set_step(QM_VCH0 - 1);
    qm_qv_st<DT, 0>(acc[1], acc[0], c);                            // epilogue of the last q | k chunk (+ store group), MFMAs of the first V chunk
    set_step(QM_VCH0);
    qm_vv<DT, 4>(acc[0], acc[1], c);
    for (int i = QM_VCH0 + 1; i < QmRow::NCH - 1; i += 2) {            // steps 41 .. 58
      set_step(i);
      qm_vv<DT, 2>(acc[1], acc[0], c);
      set_step(i + 1);
      qm_vv<DT, 2>(acc[0], acc[1], c);
    }
    set_step(QmRow::NCH - 1);
    qm_last<DT, 2>(acc[1], acc[0], c);                             // epilogue of chunk 59; the next tile's rows go out before its 2 stores
    if (!c.has_next) break;
    tile = next;
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");               // rows + statistics landed; the 2 stores behind them may fly
  }
}

}  // namespace

// idf_gemm's fused q | k | v branch tries this for the C = 640 level; IDF_BIG_UNSUPPORTED = the shape / epilogue is not this kernel's
int idf_launch_qkv640w(const idfcore::CoreParams& p, int dtype, hipStream_t s) {
  if (idf_qkv_row_knob.get() == 0) return IDF_BIG_UNSUPPORTED;
  if (!mw_row_eligible(p, dtype, R640_K, QM_N, R640_BM, 2 * R640_K) || !mw_row_vt_eligible(p)) return IDF_BIG_UNSUPPORTED;
  if (p.vt_col0 != 2 * R640_K || p.epi != (IDF_EPI_BIAS | IDF_EPI_LN_ROW)) return IDF_BIG_UNSUPPORTED;
  QmParams q;
  q.x = p.A; q.ldx = p.lda; q.ln_stats = p.ln_stats; q.w = p.W; q.ldw = p.ldw; q.c = p.ln_c; q.d = p.bias;
  q.out = static_cast<unsigned short*>(p.out); q.ldo = p.ldo; q.vt = p.vt_out; q.ld_vt = p.ld_vt; q.M = p.M;
  return dtype == IDF_BF16 ? mw_row_launch<QmParams, qkv640w_kernel<IDF_BF16>, QM_SMEM, R640_BM>(q, s)
                           : mw_row_launch<QmParams, qkv640w_kernel<IDF_F16>, QM_SMEM, R640_BM>(q, s);
}
