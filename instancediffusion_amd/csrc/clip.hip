// clip.hip -- the two kernels the CLIP text transformer (ldm/modules/encoders/modules.py:144-172, FrozenCLIPEmbedder -> Hugging Face
// CLIPTextModel) needs beside idf_gemm / idf_layernorm: causal self-attention at head dim 64 over at most 128 positions, and the
// token + position embedding gather; and the two the CLIP image tower (eval/eval_attribute_binding.py, CLIPModel.get_image_features)
// adds: bidirectional attention over at most 288 positions (idf_attention_qkv) and the patch matrix (idf_clip_patchify), both
// further down.  gfx950 only.
//
// idf_attention_causal.  One 4-wave workgroup per (sequence, head); 1-D grid, heads of one sequence adjacent (they read disjoint
// 128-B lines of the same qkv rows).  The whole K [T][64] and V^T [64][T] of the head sit in LDS (35 KB static: four workgroups per
// CU); a wave owns 16-query tiles (MFMA 16x16x32: T = 77 pads to 80 rows, on 32x32 tiles it would pad to 96) and walks the keys in
// chunks of 32 up to its diagonal:
//   S^T[key][query] = K . Q^T      two 16-key MFMA tiles x (d = 64 = 2 K-steps); a 16-key tile wholly above the diagonal is skipped;
//   softmax                         online, fp32, lane-local: the S^T accumulator puts ONE query in a lane (column l & 15) and its
//                                   keys in the 4 registers x 4 lane groups, so max / sum are 8 register ops + 2 cross-lane steps;
//   O^T[e][query] += V^T . P^T      P rounded to the 16-bit type; the two S^T tiles of a chunk ARE the B operand of the 32-deep MFMA
//                                   (lane group g holds keys 4g..4g+3 and 16+4g..16+4g+3: a permutation of the k index, applied to
//                                   the V^T fragment as well -- two 8-B LDS reads), no transpose of P anywhere.
// Masking is by select (-inf before the exponential), never arithmetic: rows <= p do not depend on anything at positions > p, bit
// for bit.  Key rows / V^T columns in [T, ceil32(T)) are zero-filled in LDS; query rows >= T compute on row T - 1 and store nothing.
#include "common.h"

namespace {

constexpr int CA_TMAX = 128;
constexpr int CA_KSTR = 72;     // 16-bit elements per K row in LDS (64 + 8: 16-B aligned rows, bank-spread)
constexpr int CA_VSTR = 132;    // per V^T row (128 + 4: 8-B aligned rows)

template <int DT> __device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (DT == IDF_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}

template <int DT>
__global__ __launch_bounds__(256) void attn_causal_kernel(const unsigned short* __restrict__ qkv, int ld, unsigned short* __restrict__ out,
                                                          int ldo, int T, int H, float scale_log2) {
  __shared__ __attribute__((aligned(16))) unsigned short Ks[CA_TMAX * CA_KSTR];
  __shared__ __attribute__((aligned(16))) unsigned short Vt[64 * CA_VSTR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int C = H * 64;
  const unsigned short* qg = qkv + (size_t)b * T * ld + h * 64;
  const unsigned short* kg = qg + C;
  const unsigned short* vg = qg + 2 * C;
  const int T32 = (T + 31) & ~31;                            // <= 128: every 32-key chunk a wave touches is initialised
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  for (int i = tid; i < T32 * 8; i += 256) {                 // K rows, 16 B per thread
    const int r = i >> 3, c = i & 7;
    u32x4 v = zero4;
    if (r < T) v = *reinterpret_cast<const u32x4*>(kg + (size_t)r * ld + c * 8);
    *reinterpret_cast<u32x4*>(Ks + r * CA_KSTR + c * 8) = v;
  }
  unsigned* Vt32 = reinterpret_cast<unsigned*>(Vt);          // V^T: a thread transposes 8 channels of a key PAIR -> 8 dword stores
  for (int i = tid; i < (T32 >> 1) * 8; i += 256) {
    const int pr = i >> 3, c = i & 7, r0 = 2 * pr;
    u32x4 v0 = zero4, v1 = zero4;
    if (r0 < T) v0 = *reinterpret_cast<const u32x4*>(vg + (size_t)r0 * ld + c * 8);
    if (r0 + 1 < T) v1 = *reinterpret_cast<const u32x4*>(vg + (size_t)(r0 + 1) * ld + c * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Vt32[(8 * c + 2 * j) * (CA_VSTR / 2) + pr] = (v0[j] & 0xffffu) | (v1[j] << 16);
      Vt32[(8 * c + 2 * j + 1) * (CA_VSTR / 2) + pr] = (v0[j] >> 16) | (v1[j] & 0xffff0000u);
    }
  }
  __syncthreads();                                           // the only barrier: the waves' trip counts differ from here on

  const int l15 = lane & 15, g = lane >> 4;
  const int nqt = (T + 15) >> 4;
  for (int qt = nqt - 1 - wave; qt >= 0; qt -= 4) {          // longest tiles first
    const int q0 = qt * 16, q = q0 + l15;
    const int qc = q < T ? q : T - 1;
    u32x4 qf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[kk] = *reinterpret_cast<const u32x4*>(qg + (size_t)qc * ld + kk * 32 + g * 8);
    f32x4 o[4];
#pragma unroll
    for (int et = 0; et < 4; ++et) o[et] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.0f;
    const int nch = (q0 >> 5) + 1;                           // chunks whose first key is <= the tile's first query
    for (int c = 0; c < nch; ++c) {
      float s[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int kb = 32 * c + 16 * t;
        if (kb <= q0) {                                      // wave-uniform: a 16-key tile wholly above the diagonal is skipped
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + (kb + l15) * CA_KSTR + kk * 32 + g * 8);
            acc = mfma16<DT>(kf, qf[kk], acc);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) s[4 * t + i] = (kb + 4 * g + i <= q) ? acc[i] * scale_log2 : -INFINITY;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) s[4 * t + i] = -INFINITY;
        }
      }
      // key 32 c <= q0 <= q is visible to every query of the tile: the chunk maximum is finite
      float mx = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // first chunk: exp2(-inf) = 0
      u32x4 pf;
      float rs = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned pk = pack2<DT>(__builtin_amdgcn_exp2f(s[2 * i] - m_new), __builtin_amdgcn_exp2f(s[2 * i + 1] - m_new));
        pf[i] = pk;
        rs += Elem<DT>::to_f32((unsigned short)(pk & 0xffffu)) + Elem<DT>::to_f32((unsigned short)(pk >> 16));   // the P that multiplies V
      }
      rs += __shfl_xor(rs, 16, 64);
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run * alpha + rs;
      m_run = m_new;
#pragma unroll
      for (int et = 0; et < 4; ++et) {
        const unsigned short* vrow = Vt + (16 * et + l15) * CA_VSTR + 32 * c + 4 * g;
        const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow), hi = *reinterpret_cast<const u32x2*>(vrow + 16);
        const u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
        for (int i = 0; i < 4; ++i) o[et][i] *= alpha;
        o[et] = mfma16<DT>(vf, pf, o[et]);
      }
    }
    if (q < T) {
      const float inv = 1.0f / l_run;
      unsigned short* op = out + ((size_t)b * T + q) * ldo + h * 64 + 4 * g;
#pragma unroll
      for (int et = 0; et < 4; ++et)
        *reinterpret_cast<u32x2*>(op + 16 * et) = u32x2{pack2<DT>(o[et][0] * inv, o[et][1] * inv), pack2<DT>(o[et][2] * inv, o[et][3] * inv)};
    }
  }
}

// out[b T + t][:] = tok_emb[clamp(ids[b][t])][:] + pos_emb[t][:], fp32 sum, one rounding.  One thread per 8 channels.
template <int DT>
__global__ __launch_bounds__(256) void clip_embed_kernel(const int* __restrict__ ids, const unsigned short* __restrict__ tok,
                                                         const unsigned short* __restrict__ pos, unsigned short* __restrict__ out, int ldo,
                                                         long long rows, int T, int C8, int vocab) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C8) return;
  const long long r = i / C8;
  const int c = (int)(i - r * C8) * 8, t = (int)(r % T);
  int id = ids[r];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  float a[8], p[8];
  unpack8<DT>(*reinterpret_cast<const u32x4*>(tok + (size_t)id * (C8 * 8) + c), a);
  unpack8<DT>(*reinterpret_cast<const u32x4*>(pos + (size_t)t * (C8 * 8) + c), p);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] += p[e];
  *reinterpret_cast<u32x4*>(out + (size_t)r * ldo + c) = pack8<DT>(a);
}

// idf_attention_qkv: the bidirectional sibling (CLIP image tower, T = 257 at ViT-L/14 224 px).  Same tiles, same lane-local online
// softmax and the same P-in-registers P.V as attn_causal_kernel; what differs:
//   * every 16-query tile walks ALL ceil32(T) / 32 key chunks, the waves take the tiles round-robin (equal trip counts);
//   * the two LDS images are sized by the call, K [T32][72] then V^T [64][T32 + 4] in dynamic LDS (T32 = ceil32(T)): 77 KB at
//     QA_TMAX = 288 -- above the static limit, two workgroups per CU still fit the 160 KB -- and 9.2 KB at T = 17;
//   * the only mask is the pad one: keys in [T, T32) are zero in LDS and -inf by select before the exponential; a 16-key tile that
//     is all padding (the second tile of the last chunk at T = 257 = 8 * 32 + 1) is skipped.  The first tile of a chunk always holds
//     a real key, so the chunk maximum is finite.
constexpr int QA_TMAX = 288;
constexpr int QA_LDS_MAX = (QA_TMAX * CA_KSTR + 64 * (QA_TMAX + 4)) * 2;      // 78848 B

template <int DT>
__global__ __launch_bounds__(256) void attn_qkv_kernel(const unsigned short* __restrict__ qkv, int ld, unsigned short* __restrict__ out,
                                                       int ldo, int T, int H, float scale_log2) {
  extern __shared__ __attribute__((aligned(16))) unsigned short qa_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int C = H * 64;
  const unsigned short* qg = qkv + (size_t)b * T * ld + h * 64;
  const unsigned short* kg = qg + C;
  const unsigned short* vg = qg + 2 * C;
  const int T32 = (T + 31) & ~31;                            // <= QA_TMAX (checked by the host): the extent of both LDS images
  const int vstr = T32 + 4;                                  // 16-bit elements per V^T row: 8-B aligned rows
  unsigned short* Ks = qa_lds;                               // [T32][CA_KSTR]; T32 * 144 B keeps V^T 16-B aligned
  unsigned short* Vt = qa_lds + T32 * CA_KSTR;               // [64][vstr]
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  for (int i = tid; i < T32 * 8; i += 256) {                 // K rows, 16 B per thread; rows >= T are zero, never read from memory
    const int r = i >> 3, c = i & 7;
    u32x4 v = zero4;
    if (r < T) v = *reinterpret_cast<const u32x4*>(kg + (size_t)r * ld + c * 8);
    *reinterpret_cast<u32x4*>(Ks + r * CA_KSTR + c * 8) = v;
  }
  unsigned* Vt32 = reinterpret_cast<unsigned*>(Vt);          // V^T: a thread transposes 8 channels of a key PAIR -> 8 dword stores
  const int vstr2 = vstr >> 1;
  for (int i = tid; i < (T32 >> 1) * 8; i += 256) {
    const int pr = i >> 3, c = i & 7, r0 = 2 * pr;
    u32x4 v0 = zero4, v1 = zero4;
    if (r0 < T) v0 = *reinterpret_cast<const u32x4*>(vg + (size_t)r0 * ld + c * 8);
    if (r0 + 1 < T) v1 = *reinterpret_cast<const u32x4*>(vg + (size_t)(r0 + 1) * ld + c * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Vt32[(8 * c + 2 * j) * vstr2 + pr] = (v0[j] & 0xffffu) | (v1[j] << 16);
      Vt32[(8 * c + 2 * j + 1) * vstr2 + pr] = (v0[j] >> 16) | (v1[j] & 0xffff0000u);
    }
  }
  __syncthreads();                                           // the only barrier

  const int l15 = lane & 15, g = lane >> 4;
  const int nqt = (T + 15) >> 4, nch = T32 >> 5;
  for (int qt = wave; qt < nqt; qt += 4) {
    const int q = qt * 16 + l15;
    const int qc = q < T ? q : T - 1;                        // a pad query computes on the last real row and stores nothing
    u32x4 qf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[kk] = *reinterpret_cast<const u32x4*>(qg + (size_t)qc * ld + kk * 32 + g * 8);
    f32x4 o[4];
#pragma unroll
    for (int et = 0; et < 4; ++et) o[et] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.0f;
    for (int c = 0; c < nch; ++c) {
      float s[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int kb = 32 * c + 16 * t;
        if (kb < T) {                                        // block-uniform: a 16-key tile that is all padding is skipped
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + (kb + l15) * CA_KSTR + kk * 32 + g * 8);
            acc = mfma16<DT>(kf, qf[kk], acc);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) s[4 * t + i] = (kb + 4 * g + i < T) ? acc[i] * scale_log2 : -INFINITY;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) s[4 * t + i] = -INFINITY;
        }
      }
      // key 32 c < T is real: the chunk maximum is finite
      float mx = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);     // first chunk: exp2(-inf) = 0
      u32x4 pf;
      float rs = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned pk = pack2<DT>(__builtin_amdgcn_exp2f(s[2 * i] - m_new), __builtin_amdgcn_exp2f(s[2 * i + 1] - m_new));
        pf[i] = pk;
        rs += Elem<DT>::to_f32((unsigned short)(pk & 0xffffu)) + Elem<DT>::to_f32((unsigned short)(pk >> 16));   // the P that multiplies V
      }
      rs += __shfl_xor(rs, 16, 64);
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run * alpha + rs;
      m_run = m_new;
#pragma unroll
      for (int et = 0; et < 4; ++et) {
        const unsigned short* vrow = Vt + (16 * et + l15) * vstr + 32 * c + 4 * g;
        const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow), hi = *reinterpret_cast<const u32x2*>(vrow + 16);
        const u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
        for (int i = 0; i < 4; ++i) o[et][i] *= alpha;
        o[et] = mfma16<DT>(vf, pf, o[et]);
      }
    }
    if (q < T) {
      const float inv = 1.0f / l_run;
      unsigned short* op = out + ((size_t)b * T + q) * ldo + h * 64 + 4 * g;
#pragma unroll
      for (int et = 0; et < 4; ++et)
        *reinterpret_cast<u32x2*>(op + 16 * et) = u32x2{pack2<DT>(o[et][0] * inv, o[et][1] * inv), pack2<DT>(o[et][2] * inv, o[et][3] * inv)};
    }
  }
}

// idf_clip_patchify: one thread per 8 output elements.  Items [0, B G^2 Kp/8) are the patch matrix -- patches[(b G + gy) G + gx]
// [c P P + ky P + kx] = pixels[b][c][gy P + ky][gx P + kx], one rounding, zero in the columns >= 3 P P -- and the B C/8 items
// behind them copy cls_row to x[b * (G^2 + 1)].
template <int DT>
__global__ __launch_bounds__(256) void clip_patchify_kernel(const float* __restrict__ px, unsigned short* __restrict__ patches, int ldp,
                                                            const unsigned short* __restrict__ cls, unsigned short* __restrict__ x, int ldx,
                                                            int B, int S, int P, int G, int Kp8, int C8) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long npatch = (long long)B * G * G * Kp8;
  if (i < npatch) {
    const long long r = i / Kp8;
    const int col0 = (int)(i - r * Kp8) * 8;
    const int b = (int)(r / (G * G)), pi = (int)(r - (long long)b * G * G), gy = pi / G, gx = pi - gy * G;
    const int PP = P * P;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = col0 + e;
      float v = 0.0f;
      if (col < 3 * PP) {
        const int c = col / PP, rem = col - c * PP, ky = rem / P, kx = rem - ky * P;
        v = px[(((size_t)b * 3 + c) * S + gy * P + ky) * S + gx * P + kx];
      }
      a[e] = v;
    }
    *reinterpret_cast<u32x4*>(patches + (size_t)r * ldp + col0) = pack8<DT>(a);
  } else if (i < npatch + (long long)B * C8) {
    const long long j = i - npatch;
    const int b = (int)(j / C8), c = (int)(j - (long long)b * C8) * 8;
    *reinterpret_cast<u32x4*>(x + (size_t)b * (G * G + 1) * ldx + c) = *reinterpret_cast<const u32x4*>(cls + c);
  }
}

// the argument contract of idf_attention_causal / idf_attention_qkv (packed [B T][q | k | v] rows, d = 64, T <= tmax)
int check_qkv_args(const void* qkv, int ld, const void* out, int ldo, int B, int T, int H, int d, float scale, int dtype, int tmax) {
  if (!qkv || !out || B <= 0 || T <= 0 || H <= 0 || d <= 0 || !(scale > 0.0f)) return IDF_E_ARG;
  if ((long long)ld < 3ll * H * d || (long long)ldo < (long long)H * d || (long long)B * H > 0x7fffffffll) return IDF_E_ARG;
  if (d != 64 || T > tmax || (dtype != IDF_BF16 && dtype != IDF_F16)) return IDF_E_UNSUPPORTED;
  if ((ld % 8) || (ldo % 8) || !aligned16(qkv) || !aligned16(out)) return IDF_E_ALIGN;
  return 0;
}

}  // namespace

extern "C" int idf_attention_causal(const void* qkv, int ld, void* out, int ldo, int B, int T, int H, int d, float scale, int dtype,
                                    void* stream) {
  if (const int e = check_qkv_args(qkv, ld, out, ldo, B, T, H, d, scale, dtype, CA_TMAX)) return e;
  hipStream_t s = (hipStream_t)stream;
  const float sl2 = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)(B * H));
  if (dtype == IDF_BF16)
    hipLaunchKernelGGL(attn_causal_kernel<IDF_BF16>, grid, dim3(256), 0, s, (const unsigned short*)qkv, ld, (unsigned short*)out, ldo, T, H, sl2);
  else
    hipLaunchKernelGGL(attn_causal_kernel<IDF_F16>, grid, dim3(256), 0, s, (const unsigned short*)qkv, ld, (unsigned short*)out, ldo, T, H, sl2);
  return idf_launch_status();
}

extern "C" int idf_clip_embed(const int* ids, const void* tok_emb, const void* pos_emb, void* out, int ldo, int B, int T, int C, int vocab,
                              int dtype, void* stream) {
  if (!ids || !tok_emb || !pos_emb || !out || B <= 0 || T <= 0 || C <= 0 || vocab <= 0 || ldo < C) return IDF_E_ARG;
  if (dtype != IDF_BF16 && dtype != IDF_F16) return IDF_E_UNSUPPORTED;
  if ((C % 8) || (ldo % 8) || !aligned16(tok_emb) || !aligned16(pos_emb) || !aligned16(out)) return IDF_E_ALIGN;
  const long long rows = (long long)B * T, n = rows * (C / 8);
  if ((n + 255) / 256 > 0x7fffffffll) return IDF_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == IDF_BF16)
    hipLaunchKernelGGL(clip_embed_kernel<IDF_BF16>, grid, dim3(256), 0, s, ids, (const unsigned short*)tok_emb, (const unsigned short*)pos_emb,
                       (unsigned short*)out, ldo, rows, T, C / 8, vocab);
  else
    hipLaunchKernelGGL(clip_embed_kernel<IDF_F16>, grid, dim3(256), 0, s, ids, (const unsigned short*)tok_emb, (const unsigned short*)pos_emb,
                       (unsigned short*)out, ldo, rows, T, C / 8, vocab);
  return idf_launch_status();
}

extern "C" int idf_attention_qkv(const void* qkv, int ld, void* out, int ldo, int B, int T, int H, int d, float scale, int dtype,
                                 void* stream) {
  if (const int e = check_qkv_args(qkv, ld, out, ldo, B, T, H, d, scale, dtype, QA_TMAX)) return e;
  hipStream_t s = (hipStream_t)stream;
  const float sl2 = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)(B * H));
  const int T32 = (T + 31) & ~31;
  const int smem = (T32 * CA_KSTR + 64 * (T32 + 4)) * 2;
  void (*kern)(const unsigned short*, int, unsigned short*, int, int, int, float) =
      dtype == IDF_BF16 ? attn_qkv_kernel<IDF_BF16> : attn_qkv_kernel<IDF_F16>;
  static std::atomic<unsigned long long> attr_done[2];
  if (const int e = idf_lds_optin(reinterpret_cast<const void*>(kern), QA_LDS_MAX, attr_done[dtype == IDF_BF16 ? 0 : 1])) return e;
  hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, (const unsigned short*)qkv, ld, (unsigned short*)out, ldo, T, H, sl2);
  return idf_launch_status();
}

extern "C" int idf_clip_patchify(const float* pixels, void* patches, int ldp, const void* cls_row, void* x, int ldx, int B, int S, int P,
                                 int C, int dtype, void* stream) {
  if (!pixels || !patches || !cls_row || !x || B <= 0 || S <= 0 || P <= 0 || P > 32 || (S % P) || C <= 0 || ldx < C) return IDF_E_ARG;
  const int G = S / P, Kp = (3 * P * P + 63) & ~63;
  if (ldp < Kp) return IDF_E_ARG;
  if (dtype != IDF_BF16 && dtype != IDF_F16) return IDF_E_UNSUPPORTED;
  if ((C % 8) || (ldx % 8) || (ldp % 8) || !aligned16(patches) || !aligned16(cls_row) || !aligned16(x) || (((uintptr_t)pixels) & 3u))
    return IDF_E_ALIGN;
  const long long n = (long long)B * G * G * (Kp / 8) + (long long)B * (C / 8);
  if ((n + 255) / 256 > 0x7fffffffll || (long long)B * (G * G + 1) > 0x7fffffffll) return IDF_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == IDF_BF16)
    hipLaunchKernelGGL(clip_patchify_kernel<IDF_BF16>, grid, dim3(256), 0, s, pixels, (unsigned short*)patches, ldp,
                       (const unsigned short*)cls_row, (unsigned short*)x, ldx, B, S, P, G, Kp / 8, C / 8);
  else
    hipLaunchKernelGGL(clip_patchify_kernel<IDF_F16>, grid, dim3(256), 0, s, pixels, (unsigned short*)patches, ldp,
                       (const unsigned short*)cls_row, (unsigned short*)x, ldx, B, S, P, G, Kp / 8, C / 8);
  return idf_launch_status();
}
