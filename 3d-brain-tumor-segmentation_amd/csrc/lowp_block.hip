// The ResnetBlock's own passes on 16-bit tensors: column sums (the squeeze), the block epilogue (alone and with the output head in it),
// the gate backward and the fused gate + GroupNorm-2 backward.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.h"
#include "bts_internal.h"
#include "lowp_common.h"
#include "finalize_parts.h"

// ---- global average pool of the shortcut (resnet.py:45-46,121): per (n, channel) mean over the voxels, fp64 partials
template <typename T>
__global__ __launch_bounds__(256) void lp_colsum_kernel(const unsigned short* x, double* partial, long V, int C, int B) {
  // block (b, n): voxels [b*per, ...) ; thread t handles channel octet (t % (C/8)) of every (256 / (C/8))-th voxel
  const int n = blockIdx.y;
  const int oct = C / 8;
  const int co = threadIdx.x % oct, vr = threadIdx.x / oct, vstep = 256 / oct;
  const long per = (V + B - 1) / B;
  const long a = (long)blockIdx.x * per, bnd = (a + per < V) ? a + per : V;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float fs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int cnt = 0;
  if (vr < vstep) {
    for (long v = a + vr; v < bnd; v += vstep) {
      float t[8];
      unpack8<T>(*reinterpret_cast<const u32x4*>(x + ((long)n * V + v) * C + co * 8), t);
#pragma unroll
      for (int e = 0; e < 8; ++e) fs[e] += t[e];
      if (++cnt == 256) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] += fs[e]; fs[e] = 0.f; }
        cnt = 0;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] += fs[e];
  // combine the vstep voxel-rows through LDS in fixed order
  __shared__ double sh[256 * 8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sh[threadIdx.x * 8 + e] = (vr < vstep) ? s[e] : 0.0;
  __syncthreads();
  if (threadIdx.x < C) {
    const int c = threadIdx.x, o = c / 8, e = c % 8;
    double tot = 0.0;
    for (int r = 0; r < vstep; ++r) tot += sh[(r * oct + o) * 8 + e];
    partial[((long)n * B + blockIdx.x) * C + c] = tot;
  }
}
__global__ __launch_bounds__(256) void lp_colsum_finalize_kernel(const double* partial, float* out, int N, int C, int B, double scale) {
  // one wave per (n, c): lanes split the blocks, fixed-order shuffle tree
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N * C) return;
  const int n = i / C, c = i % C;
  double s = 0.0;
  for (int b = lane; b < B; b += 64) s += partial[((long)n * B + b) * C + c];
  s = wave_sum_f64(s);
  if (lane == 0) out[i] = (float)(s * scale);
}
int bts_lp_colsum_finalize_(const double* partial, float* out, int N, int C, int B, double scale, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(lp_colsum_finalize_kernel, dim3((N * C + 3) / 4), dim3(256), 0, stream, partial, out, N, C, B, scale);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
static int lp_colsum_blocks(long V) {
  long b = V / 2048;
  if (b < 1) b = 1;
  if (b > 512) b = 512;
  return (int)b;
}
extern "C" long bts_lp_colsum_workspace(int N, long V, int C) {
  if (N <= 0 || V <= 0 || C <= 0) return -1;
  return (long)N * lp_colsum_blocks(V) * C * 8 + 64;
}
extern "C" int bts_lp_colsum(int dtype, const void* x, float* out, void* workspace, long workspace_bytes, int N, long V, int C, float scale,
                             hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || C <= 0 || C % 8 != 0 || C > 256 || 256 % (C / 8) != 0) return BTS_ERR_SHAPE;
  if (((uintptr_t)x) & 15) return BTS_ERR_ALIGN;
  const int B = lp_colsum_blocks(V);
  if (workspace_bytes < bts_lp_colsum_workspace(N, V, C)) return BTS_ERR_WORKSPACE;
  double* partial = reinterpret_cast<double*>(workspace);
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_colsum_kernel<decltype(t)>, dim3(B, N), dim3(256), 0, stream, (const unsigned short*)x, partial, V, C, B);
  });
  BTS_LAUNCH_CHECK();
  return bts_lp_colsum_finalize_(partial, out, N, C, B, (double)scale, stream);
}

// ---- ResNet block epilogue (resnet.py:127-137): out = res * (sigmoid(res . w_sp) + ch[n]) + relu(GN2(c2))
// one voxel per group of C/8 lanes: the spatial dot product is reduced across those lanes with xor shuffles
template <typename T>
__global__ __launch_bounds__(256) void lp_block_epilogue_kernel(const unsigned short* res, const unsigned short* c2, unsigned short* out,
                                                                float* sp_out, const float* wsp, const float* ch, const float* gamma, const float* beta,
                                                                const float* mean, const float* rstd, long total8, long E, long L, int C,
                                                                int G, int cg, int ldo, int mode) {
  const int oct = C / 8;
  for (long f = blockIdx.x * 256L + threadIdx.x; f < total8; f += (long)gridDim.x * 256) {
    const long i = f * 8;
    const long n = i / E;
    const long r = i - n * E;
    const int c = (int)(r % C);
    const long pix = i / C;
    float a[8], b[8], o[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(res + i), a);
    unpack8<T>(*reinterpret_cast<const u32x4*>(c2 + i), b);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(a[e], wsp[c + e], dot);
    dot = lane_group_sum_f32(dot, oct);   // (oct is a power of two <= 32; lanes of a voxel are adjacent)
    const float sp = 1.f / (1.f + __expf(-dot));
    if (sp_out != nullptr && c == 0) sp_out[pix] = sp;   // the spatial gate, kept for the backward pass (resnet.py:127)
    const int gsl = (int)(r / L);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int g = (mode == BTS_GN_SLAB) ? gsl : (c + e) / cg;
      const int idx = (mode == BTS_GN_SLAB) ? g * cg + ((c + e) % cg) : (c + e);
      const float t = fmaxf((b[e] - mean[n * G + g]) * rstd[n * G + g] * gamma[idx] + beta[idx], 0.f);
      o[e] = fmaf(a[e], sp + ch[n * C + c + e], t);
    }
    *reinterpret_cast<u32x4*>(out + pix * ldo + c) = pack8<T>(o);
  }
}
// chunked form (see lp_gn_apply_chunk_kernel): per-thread channels fixed, gate weights / statistics / scales in registers
template <typename T>
__global__ __launch_bounds__(256) void lp_block_epilogue_chunk_kernel(const unsigned short* __restrict__ res, const unsigned short* __restrict__ c2,
                                                                      unsigned short* __restrict__ out, float* __restrict__ sp_out,
                                                                      const float* __restrict__ wsp, const float* __restrict__ ch,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd, long Lu,
                                                                      long per, int C, int G, int cg, int ldo, int slab, int upn) {
  const int unit = blockIdx.y, n = unit / upn, u = unit - n * upn;
  const long lo = (long)unit * Lu;
  const long a = lo + (long)blockIdx.x * per;
  const long bnd = (a + per < lo + Lu) ? a + per : lo + Lu;
  const int t8 = threadIdx.x * 8, c = t8 % C, oct = C / 8;
  float mu[8], sc[8], be[8], ws[8], cw[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int g = slab ? u : (c + e) / cg;
    const int idx = slab ? g * cg + ((c + e) % cg) : (c + e);
    mu[e] = mean[n * G + g];
    sc[e] = rstd[n * G + g] * gamma[idx];
    be[e] = beta[idx];
    ws[e] = wsp[c + e];
    cw[e] = ch[n * C + c + e];
  }
  const long pstep = 2048 / C;
  const long pix = a / C + t8 / C;
  const unsigned short* ra = res + a + t8;
  const unsigned short* rb = c2 + a + t8;
  const long K = (bnd - a) / 2048;
  auto one = [&](const u32x4 r0, const u32x4 r1, long px) {
    float va[8], vb[8], o[8];
    unpack8<T>(r0, va);
    unpack8<T>(r1, vb);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(va[e], ws[e], dot);
    dot = lane_group_sum_f32(dot, oct);
    const float sp = 1.f / (1.f + __expf(-dot));
    if (sp_out != nullptr && c == 0) sp_out[px] = sp;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = fmaxf(fmaf(vb[e] - mu[e], sc[e], be[e]), 0.f);
      o[e] = fmaf(va[e], sp + cw[e], t);
    }
    *reinterpret_cast<u32x4*>(out + px * ldo + c) = pack8<T>(o);
  };
  long k = 0;
  for (; k + 2 <= K; k += 2) {
    u32x4 r0[2], r1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      r0[j] = *reinterpret_cast<const u32x4*>(ra + (k + j) * 2048);
      r1[j] = *reinterpret_cast<const u32x4*>(rb + (k + j) * 2048);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) one(r0[j], r1[j], pix + (k + j) * pstep);
  }
  for (; k < K; ++k) one(*reinterpret_cast<const u32x4*>(ra + k * 2048), *reinterpret_cast<const u32x4*>(rb + k * 2048), pix + k * pstep);
}
extern "C" int bts_lp_block_epilogue(int dtype, const void* res, const void* c2, void* out, float* sp_out, const float* wsp, const float* ch,
                                     const float* gamma, const float* beta, const float* mean, const float* rstd, int N, long V, int C,
                                     int ldo, int G, int mode, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || C <= 0 || G <= 0 || C % 8 != 0 || C > 256 || ((C / 8) & (C / 8 - 1)) != 0 || C % G != 0 || ldo % 8 != 0 || ldo < C) return BTS_ERR_SHAPE;
  const long E = V * C, L = E / G;
  if (mode == BTS_GN_SLAB && L % 8 != 0) return BTS_ERR_UNSUPPORTED;
  if ((((uintptr_t)res) & 15) || (((uintptr_t)c2) & 15) || (((uintptr_t)out) & 15)) return BTS_ERR_ALIGN;
  (void)hipGetLastError();
  {
    const int slab = mode == BTS_GN_SLAB;
    const long Lu = slab ? L : E;
    if (2048 % C == 0 && Lu % 2048 == 0) {
      const int upn = slab ? G : 1;
      int B;
      const long per = lp_chunk_per(Lu, (long)N * upn, &B);
      const dim3 grid((unsigned)B, (unsigned)(N * upn));
      lp_typed(dtype, [&](auto t) {
        hipLaunchKernelGGL(lp_block_epilogue_chunk_kernel<decltype(t)>, grid, dim3(256), 0, stream, (const unsigned short*)res, (const unsigned short*)c2, (unsigned short*)out, sp_out, wsp, ch, gamma, beta, mean, rstd, Lu, per, C, G, C / G, ldo, slab, upn);
      });
      BTS_LAUNCH_CHECK();
      return BTS_OK;
    }
  }
  const long total8 = (long)N * E / 8;
  // (the C/8 lanes of a voxel are adjacent and aligned inside a wave, so they enter and leave the loop together)
  long blocks = (total8 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_block_epilogue_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, stream, (const unsigned short*)res, (const unsigned short*)c2, (unsigned short*)out, sp_out, wsp, ch, gamma, beta, mean, rstd, total8, E, L, C, G, C / G, ldo, mode);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- the LAST block's epilogue with the output head in it (inference: decoder.py:55-63 after the top decoder block, model.py:63-68) ----
// y_head[v][k] = sigmoid( sum_c out[v][c] * W[c][k] + b[k] ),  out = res * (sigmoid(res . w_sp) + ch) + relu(GN2(c2)) as above -- `out` has ONE
// reader in a forward without a backward, the 1x1x1 head (32 -> 3 at the CLI defaults), so it is never written: the separate pair costs a
// write and a read of the 32-channel tensor plus a launch (160 x 192 x 160: 177 + 101 us; fused: one pass over res and c2).  The head sees the
// fp32 values of `out`, not their 16-bit roundings.  Chunked form only (its conditions as in bts_lp_block_epilogue); K <= 4.
template <typename T, int K>
__global__ __launch_bounds__(256) void lp_block_epilogue_head_kernel(const unsigned short* __restrict__ res, const unsigned short* __restrict__ c2,
                                                                     float* __restrict__ yh, const float* __restrict__ wsp, const float* __restrict__ ch,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                     const float* __restrict__ hw, const float* __restrict__ hb, long Lu, long per,
                                                                     int C, int G, int cg, int slab, int upn, int sigmoid) {
  const int unit = blockIdx.y, n = unit / upn, u = unit - n * upn;
  const long lo = (long)unit * Lu;
  const long a = lo + (long)blockIdx.x * per;
  const long bnd = (a + per < lo + Lu) ? a + per : lo + Lu;
  const int t8 = threadIdx.x * 8, c = t8 % C, oct = C / 8;
  float mu[8], sc[8], be[8], ws[8], cw[8], wr[8][K], hbk[K];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int g = slab ? u : (c + e) / cg;
    const int idx = slab ? g * cg + ((c + e) % cg) : (c + e);
    mu[e] = mean[n * G + g];
    sc[e] = rstd[n * G + g] * gamma[idx];
    be[e] = beta[idx];
    ws[e] = wsp[c + e];
    cw[e] = ch[n * C + c + e];
#pragma unroll
    for (int k = 0; k < K; ++k) wr[e][k] = hw[(c + e) * K + k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) hbk[k] = hb ? hb[k] : 0.f;
  const long pstep = 2048 / C;
  const long pix = a / C + t8 / C;
  const unsigned short* ra = res + a + t8;
  const unsigned short* rb = c2 + a + t8;
  const long Kc = (bnd - a) / 2048;
  auto one = [&](const u32x4 r0, const u32x4 r1, long px) {
    float va[8], vb[8];
    unpack8<T>(r0, va);
    unpack8<T>(r1, vb);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(va[e], ws[e], dot);
    dot = lane_group_sum_f32(dot, oct);
    const float sp = 1.f / (1.f + __expf(-dot));
    float hk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) hk[k] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = fmaxf(fmaf(vb[e] - mu[e], sc[e], be[e]), 0.f);
      const float o = fmaf(va[e], sp + cw[e], t);
#pragma unroll
      for (int k = 0; k < K; ++k) hk[k] = fmaf(o, wr[e][k], hk[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      hk[k] = lane_group_sum_f32(hk[k], oct);
    if (c == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float r = hk[k] + hbk[k];
        if (sigmoid) r = 1.f / (1.f + __expf(-r));
        yh[px * K + k] = r;
      }
    }
  };
  long k = 0;
  for (; k + 2 <= Kc; k += 2) {
    u32x4 r0[2], r1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      r0[j] = *reinterpret_cast<const u32x4*>(ra + (k + j) * 2048);
      r1[j] = *reinterpret_cast<const u32x4*>(rb + (k + j) * 2048);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) one(r0[j], r1[j], pix + (k + j) * pstep);
  }
  for (; k < Kc; ++k) one(*reinterpret_cast<const u32x4*>(ra + k * 2048), *reinterpret_cast<const u32x4*>(rb + k * 2048), pix + k * pstep);
}
extern "C" int bts_lp_block_epilogue_head(int dtype, const void* res, const void* c2, float* y_head, const float* wsp, const float* ch,
                                          const float* gamma, const float* beta, const float* mean, const float* rstd, const float* head_w,
                                          const float* head_b, int N, long V, int C, int G, int mode, int K, int sigmoid, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || C <= 0 || G <= 0 || C % 8 != 0 || C > 256 || ((C / 8) & (C / 8 - 1)) != 0 || C % G != 0 || K < 1) return BTS_ERR_SHAPE;
  const long E = V * C, L = E / G;
  const int slab = mode == BTS_GN_SLAB;
  const long Lu = slab ? L : E;
  // (per-thread state: 8 x K head weights on top of the epilogue's 40 registers -- wide blocks and heads stay on the two-kernel route)
  if (K > 4 || C > 64 || (slab && L % 8 != 0) || 2048 % C != 0 || Lu % 2048 != 0) return BTS_ERR_UNSUPPORTED;
  if ((((uintptr_t)res) & 15) || (((uintptr_t)c2) & 15) || (((uintptr_t)y_head) & 3)) return BTS_ERR_ALIGN;
  const int upn = slab ? G : 1;
  int B;
  const long per = lp_chunk_per(Lu, (long)N * upn, &B);
  const dim3 grid((unsigned)B, (unsigned)(N * upn));
  (void)hipGetLastError();
#define LP_EH(TT, K_) hipLaunchKernelGGL((lp_block_epilogue_head_kernel<TT, K_>), grid, dim3(256), 0, stream, (const unsigned short*)res, (const unsigned short*)c2, y_head, wsp, ch, gamma, beta, mean, rstd, head_w, head_b, Lu, per, C, G, C / G, slab, upn, sigmoid)
#define LP_EH_K(TT) do { if (K == 1) LP_EH(TT, 1); else if (K == 2) LP_EH(TT, 2); else if (K == 3) LP_EH(TT, 3); else LP_EH(TT, 4); } while (0)
  lp_typed(dtype, [&](auto t) { LP_EH_K(decltype(t)); });
#undef LP_EH_K
#undef LP_EH
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// =====================================================================================================================
// Gate (squeeze-excitation) backward on 16-bit tensors (resnet.py:121-130 under TF autodiff): with g = dout * res per element,
//   t_v = sum_c g, ds_v = t_v sp_v (1 - sp_v)            (spatial gate, fp32 per voxel)
//   Pch[n][c] = sum_v g, Pw[c] = sum_v ds_v res          (per-block partials, fp64, layout of se.hip; stages 2a / 2 are se.hip's)
//   dres = dout (sp + ch) + ds w_sp + dgap / V           (written in the storage type)
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void lp_se_bwd_reduce_kernel(const unsigned short* dout, const unsigned short* res, const float* sp,
                                                               float* ds_out, double* partial, long V, int F, int lddo, long vspan) {
  __shared__ double sh[256 * 16];
  const int F8 = F >> 3;
  const int vpb = 256 / F8;
  const int lg = threadIdx.x % F8, vl = threadIdx.x / F8;
  const int c = lg * 8;
  const long n = blockIdx.y;
  const long v0 = (long)blockIdx.x * vspan;
  long v1 = v0 + vspan;
  if (v1 > V) v1 = V;
  double a[8], b[8];
  float fa[8], fb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] = b[e] = 0.0; fa[e] = fb[e] = 0.f; }
  int cnt = 0;
  for (long vv = v0 + vl; vv < v1; vv += vpb) {
    const long v = n * V + vv;
    float r[8], d[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(res + v * F + c), r);
    unpack8<T>(*reinterpret_cast<const u32x4*>(dout + v * lddo + c), d);
    float t = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) t = fmaf(d[e], r[e], t);
    for (int o = F8 >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    const float s = sp[v];
    const float dsv = t * s * (1.f - s);
    if (lg == 0) ds_out[v] = dsv;
#pragma unroll
    for (int e = 0; e < 8; ++e) { fa[e] = fmaf(d[e], r[e], fa[e]); fb[e] = fmaf(dsv, r[e], fb[e]); }
    if (++cnt == 64) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] += fa[e]; b[e] += fb[e]; fa[e] = fb[e] = 0.f; }
      cnt = 0;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { sh[threadIdx.x * 16 + e] = a[e] + fa[e]; sh[threadIdx.x * 16 + 8 + e] = b[e] + fb[e]; }
  __syncthreads();
  for (int col = threadIdx.x; col < F; col += 256) {
    const int e = col & 7, l = col >> 3;
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < vpb; ++k) { sa += sh[(k * F8 + l) * 16 + e]; sb += sh[(k * F8 + l) * 16 + 8 + e]; }
    const long o = (((long)n * gridDim.x + blockIdx.x) * F + col) * 2;
    partial[o] = sa;
    partial[o + 1] = sb;
  }
}
static int lp_se_blocks(long V, int N, int F, long* vspan) {
  const int vpb = 256 / (F / 8);
  long B = (1024 + N - 1) / N;
  if (B > 512) B = 512;
  long span = (V + B - 1) / B;
  span = (span + vpb - 1) / vpb * vpb;
  *vspan = span;
  return (int)((V + span - 1) / span);
}
// =====================================================================================================================
// A ResnetBlock's gate backward and GroupNorm-2 backward in ONE pair of passes (resnet.py:121-137 under TF autodiff).  Both read the
// gradient of the block output: the separate routes (bts_lp_se_bwd, bts_lp_gn_bwd) read it four times and launch ten kernels; here
// the reduce pass reads dout, res, c2 once (GroupNorm class sums + gate sums + the per-voxel spatial-gate gradient) and the apply pass
// reads dout, c2 once and writes dres and dc2 (+ both bias-gradient rows).  Thread mapping of the GroupNorm kernels: a workgroup owns a
// span of one (n, group) unit, a thread 8 consecutive channels of a voxel, the C/8 lanes of a voxel are neighbours.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void lp_blk_bwd_reduce_kernel(const unsigned short* x, const unsigned short* dy, const unsigned short* res,
                                                                const float* sp, const float* gamma, const float* beta, const float* mean,
                                                                const float* rstd, double* partial, double* se_partial, float* ds_out, long E,
                                                                long L, long span, int C, int G, int cg, int lddy) {
  __shared__ double sh[4 * 4 * 16];
  __shared__ double sh2[256 * 16];
  const int unit = blockIdx.y, n = unit / G, g = unit % G;
  const long lo = (long)blockIdx.x * span;
  long hi = lo + span;
  if (hi > L) hi = L;
  const long ubase = (long)g * L;
  const int cph = (int)((ubase + lo + threadIdx.x * 8L) % C);
  const int F8 = C >> 3;
  float gam[8], bet[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { const int idx = g * cg + ((cph + e) % cg); gam[e] = gamma[idx]; bet[e] = beta[idx]; }
  const float m = mean[unit], rs = rstd[unit];
  double a[8], b[8], pa[8], pb[8];
  float fa[8], fb[8], qa[8], qb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] = b[e] = pa[e] = pb[e] = 0.0; fa[e] = fb[e] = qa[e] = qb[e] = 0.f; }
  const unsigned short* xb = x + (long)n * E + ubase;
  const unsigned short* rb = res + (long)n * E + ubase;
  const long pstep = 2048 / C, pix0 = ((long)n * E + ubase + lo + threadIdx.x * 8L) / C;
  int cnt = 0;
  // (hi - lo is a multiple of 2048: the lanes of a voxel leave together.)  Two steps per trip, their six loads issued first.
  auto one = [&](const u32x4 rv, const u32x4 rr, const u32x4 rd, float s, long pix) {
    float v[8], d[8], r[8];
    unpack8<T>(rv, v);
    unpack8<T>(rr, r);
    unpack8<T>(rd, d);
    float t = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) t = fmaf(d[e], r[e], t);
    for (int o = F8 >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    const float dsv = t * s * (1.f - s);
    if ((threadIdx.x & (F8 - 1)) == 0) ds_out[pix] = dsv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (v[e] - m) * rs;
      float de = d[e];
      if (!(xh * gam[e] + bet[e] > 0.f)) de = 0.f;
      fa[e] = fmaf(de, xh, fa[e]);
      fb[e] += de;
      qa[e] = fmaf(d[e], r[e], qa[e]);
      qb[e] = fmaf(dsv, r[e], qb[e]);
    }
    if (++cnt == 32) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] += fa[e]; b[e] += fb[e]; pa[e] += qa[e]; pb[e] += qb[e]; fa[e] = fb[e] = qa[e] = qb[e] = 0.f; }
      cnt = 0;
    }
  };
  {
    const long K = (hi - lo) / 2048;
    const long i0 = lo + threadIdx.x * 8L;
    long k = 0;
    for (; k + 2 <= K; k += 2) {
      u32x4 rv[2], rr[2], rd[2];
      float s[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long i = i0 + (k + j) * 2048, pix = pix0 + (k + j) * pstep;
        rv[j] = *reinterpret_cast<const u32x4*>(xb + i);
        rr[j] = *reinterpret_cast<const u32x4*>(rb + i);
        rd[j] = *reinterpret_cast<const u32x4*>(dy + pix * lddy + cph);
        s[j] = sp[pix];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) one(rv[j], rr[j], rd[j], s[j], pix0 + (k + j) * pstep);
    }
    for (; k < K; ++k) {
      const long i = i0 + k * 2048, pix = pix0 + k * pstep;
      one(*reinterpret_cast<const u32x4*>(xb + i), *reinterpret_cast<const u32x4*>(rb + i), *reinterpret_cast<const u32x4*>(dy + pix * lddy + cph), sp[pix], pix);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] += fa[e]; b[e] += fb[e]; pa[e] += qa[e]; pb[e] += qb[e]; }
  // gate sums first (their LDS array is separate): threads of equal octet (t mod F8) in thread order
#pragma unroll
  for (int e = 0; e < 8; ++e) { sh2[threadIdx.x * 16 + e] = pa[e]; sh2[threadIdx.x * 16 + 8 + e] = pb[e]; }
  // GroupNorm class sums exactly as lp_gn_bwd_reduce_kernel
  const int p = cg > 8 ? cg / 8 : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 32; off >= p; off >>= 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] += __shfl_xor(a[e], off, 64); b[e] += __shfl_xor(b[e], off, 64); }
  }
  if (lane < p) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { sh[((wave * 4 + lane) * 8 + e) * 2] = a[e]; sh[((wave * 4 + lane) * 8 + e) * 2 + 1] = b[e]; }
  }
  __syncthreads();
  if (threadIdx.x < cg) {
    const int j = threadIdx.x;
    const int cph0 = (int)((ubase + lo) % C);
    double sa = 0.0, sb = 0.0;
    for (int w = 0; w < 4; ++w)
      for (int q = 0; q < p; ++q)
        for (int e = 0; e < 8; ++e)
          if (((cph0 + 8 * q + e) % cg) == j) { sa += sh[((w * 4 + q) * 8 + e) * 2]; sb += sh[((w * 4 + q) * 8 + e) * 2 + 1]; }
    double* o = partial + (((long)unit * gridDim.x + blockIdx.x) * cg + j) * 2;
    o[0] = sa; o[1] = sb;
  }
  const int vpb = 256 / F8;
  for (int col = threadIdx.x; col < C; col += 256) {
    const int e = col & 7, l = col >> 3;
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < vpb; ++k) { sa += sh2[(k * F8 + l) * 16 + e]; sb += sh2[(k * F8 + l) * 16 + 8 + e]; }
    const long o = ((((long)n * G + g) * gridDim.x + blockIdx.x) * C + col) * 2;      // block index inside the sample: g * B + b
    se_partial[o] = sa;
    se_partial[o + 1] = sb;
  }
}
template <typename T>
__global__ __launch_bounds__(256) void lp_blk_bwd_apply_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
                                                               unsigned short* __restrict__ dx, unsigned short* __restrict__ dres,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ c1, const float* __restrict__ c2,
                                                               const float* __restrict__ sp, const float* __restrict__ ds,
                                                               const float* __restrict__ ch, const float* __restrict__ wsp,
                                                               const float* __restrict__ dgap, long L, long per, int C, int G, int cg, int lddy,
                                                               double* dbias_c2, double* dbias_pt) {
  __shared__ float dbsh[256 * 8];
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cr[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int unit = blockIdx.y, n = unit / G, g = unit - n * G;
  const long lo = (long)unit * L;
  const long a = lo + (long)blockIdx.x * per;
  const long bnd = (a + per < lo + L) ? a + per : lo + L;
  const int t8 = threadIdx.x * 8, c = t8 % C;
  float gam[8], bet[8], chv[8], wsv[8], dgv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int idx = g * cg + ((c + e) % cg);
    gam[e] = gamma[idx]; bet[e] = beta[idx];
    chv[e] = ch[n * C + c + e]; wsv[e] = wsp[c + e]; dgv[e] = dgap[n * C + c + e];
  }
  const float m = mean[unit], rs = rstd[unit], k1 = c1[unit], k2 = c2[unit];
  const long pstep = 2048 / C, pix = a / C + t8 / C;
  const long K = (bnd - a) / 2048;
  auto one = [&](const u32x4 rx, const u32x4 rd, float s, float dsv, long i) {
    float v[8], d[8], o[8], q[8];
    unpack8<T>(rx, v);
    unpack8<T>(rd, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (v[e] - m) * rs;
      float de = d[e];
      if (!(xh * gam[e] + bet[e] > 0.f)) de = 0.f;
      o[e] = (de * gam[e] - k1 - xh * k2) * rs;
      cs[e] += o[e];
      q[e] = fmaf(d[e], s + chv[e], fmaf(dsv, wsv[e], dgv[e]));
      cr[e] += q[e];
    }
    *reinterpret_cast<u32x4*>(dx + i) = pack8<T>(o);
    *reinterpret_cast<u32x4*>(dres + i) = pack8<T>(q);
  };
  long k = 0;
  for (; k + 2 <= K; k += 2) {
    u32x4 rx[2], rd[2];
    float s[2], dv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long px = pix + (k + j) * pstep;
      rx[j] = *reinterpret_cast<const u32x4*>(x + a + t8 + (k + j) * 2048);
      rd[j] = *reinterpret_cast<const u32x4*>(dy + px * lddy + c);
      s[j] = sp[px]; dv[j] = ds[px];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) one(rx[j], rd[j], s[j], dv[j], a + t8 + (k + j) * 2048);
  }
  for (; k < K; ++k) {
    const long px = pix + k * pstep;
    one(*reinterpret_cast<const u32x4*>(x + a + t8 + k * 2048), *reinterpret_cast<const u32x4*>(dy + px * lddy + c), sp[px], ds[px], a + t8 + k * 2048);
  }
  const long row = (long)blockIdx.y * gridDim.x + blockIdx.x;
  if (dbias_c2 != nullptr) lp_dbias_block(cs, 0, C / 8, dbias_c2 + row * C, dbsh);     // (launch-uniform)
  if (dbias_pt != nullptr) lp_dbias_block(cr, 0, C / 8, dbias_pt + row * C, dbsh);
}
extern "C" long bts_lp_block_bwd_workspace(int N, long V, int F, int R, int G) {
  if (N <= 0 || V <= 0 || F < 8 || R <= 0 || G <= 0 || F % G != 0) return -1;
  const long L = V * F / G;
  const long B = lp_gnb_blocks(L);
  long vspan;
  long Bse = lp_se_blocks(V, N, F, &vspan);      // (the A/B route with separate reduce passes uses the gate kernel's own block count)
  if (Bse < G * B) Bse = G * B;
  return (long)N * G * B * (F / G) * 2 * 8 + (long)N * G * 2 * 4 + 64      // GroupNorm partials, c1 / c2
         + (long)N * Bse * F * 2 * 8 + ((long)N * F * 3 + (long)N * R) * 8 + 128      // gate partials, red, scratch
         + 2 * ((N * (long)G > 2048 ? N * (long)G : 2048L) * F * 8 + 64);      // two sets of bias-gradient rows (one per apply workgroup)
}
// The two small launches of the fused block backward (see bts_lp_block_bwd).  Middle: workgroups [0, G) finish GroupNorm-2's class sums
// (lp_gn_bwd_finalize_kernel's work), the rest sum the gate partials per (n, c) (se_bwd_partial_reduce_kernel's).  Tail: workgroups [0, np)
// form the SE-MLP's parameter gradients from the per-sample pass's scratch (se_mlp_bwd_param_kernel's work), the next F finish conv2's bias
// gradient, the last F the shortcut conv's (lp_dbias_finalize_kernel's).  Same bodies, same summation order: bit-identical to the six launches.
__global__ __launch_bounds__(256) void lp_blk_bwd_middle_kernel(const double* partial, const float* gamma, float* dgamma, float* dbeta, float* c1,
                                                                float* c2, const double* se_partial, double* red, int N, int G, int B, int cg,
                                                                double L, int Bse, int F) {
  __shared__ double sh[256 * 2];
  __shared__ double tot[256 * 2];
  if ((int)blockIdx.x < G) lp_gn_bwd_finalize_body(partial, gamma, dgamma, dbeta, c1, c2, N, G, B, cg, L, 1, blockIdx.x, sh, tot);
  else se_bwd_partial_reduce_body(se_partial, red, N, Bse, F, (int)blockIdx.x - G);
}
__global__ __launch_bounds__(256) void lp_blk_bwd_tail_kernel(const double* red, const float* gap, const float* hbuf, float* dw1, float* dw2, float* dwsp,
                                                              const double* scratch, int N, int F, int R, int np, const double* dbp1, float* db1,
                                                              const double* dbp2, float* db2, int nblocks) {
  __shared__ double sh[4];
  int b = blockIdx.x;
  if (b < np) { se_mlp_bwd_param_body(red, gap, hbuf, dw1, dw2, dwsp, scratch, N, F, R, 1, b); return; }
  b -= np;
  if (db1 != nullptr) {
    if (b < F) { lp_dbias_finalize_body(dbp1, db1, nblocks, F, 1, b, sh); return; }
    b -= F;
  }
  lp_dbias_finalize_body(dbp2, db2, nblocks, F, 1, b, sh);
}
// dout (N,V,F) rows of lddo; res, c2 dense; dres, dc2 dense outputs in the storage type; ds (N*V) and dgap (N,F) fp32 scratch outputs;
// parameter gradients accumulate (+=); dbias_pt / dbias_c2 (may be NULL): the shortcut conv's / conv2's bias gradients (+=).
// BTS_ERR_UNSUPPORTED outside the kernels' tiling: the caller runs bts_lp_gn_bwd and bts_lp_se_bwd.
extern "C" int bts_lp_block_bwd(int dtype, const void* dout, int lddo, const void* res, const void* c2x, const float* sp, const float* gap,
                                const float* h, const float* ch, const float* w1, const float* w2, const float* wsp, const float* gamma,
                                const float* beta, const float* mean, const float* rstd, void* dres, void* dc2, float* ds, float* dgap, float* dw1,
                                float* dw2, float* dwsp, float* dgamma, float* dbeta, float* dbias_pt, float* dbias_c2, void* workspace,
                                long workspace_bytes, int N, long V, int F, int R, int G, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || F < 8 || G <= 0 || F < G || F % G != 0 || (F & (F - 1)) != 0 || F > 256 || lddo % 8 != 0 || lddo < F || R <= 0) return BTS_ERR_SHAPE;
  const long E = V * F, L = E / G;
  const int cg = F / G;
  if (!lp_gn_bwd_tiled(V, F, G)) return BTS_ERR_UNSUPPORTED;
  if ((((uintptr_t)dout) & 15) || (((uintptr_t)res) & 15) || (((uintptr_t)c2x) & 15) || (((uintptr_t)dres) & 15) || (((uintptr_t)dc2) & 15)) return BTS_ERR_ALIGN;
  if (workspace == nullptr || (((uintptr_t)workspace) & 15) || workspace_bytes < bts_lp_block_bwd_workspace(N, V, F, R, G)) return BTS_ERR_WORKSPACE;
  const int B = lp_gnb_blocks(L);
  const long span = ((L / 2048 + B - 1) / B) * 2048;
  double* partial = reinterpret_cast<double*>(workspace);
  float* c1 = reinterpret_cast<float*>(partial + (long)N * G * B * cg * 2);
  float* c2 = c1 + (long)N * G;
  double* sep = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(c2 + (long)N * G) + 63) & ~(uintptr_t)63);
  long vspan_se;
  long Bmax = lp_se_blocks(V, N, F, &vspan_se);
  if (Bmax < (long)G * B) Bmax = (long)G * B;
  double* red = sep + (long)N * Bmax * F * 2;
  double* scratch = red + (long)N * F * 2;
  double* dbp1 = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(scratch + (long)N * F + (long)N * R) + 63) & ~(uintptr_t)63);
  double* dbp2 = dbp1 + (N * (long)G > 2048 ? N * (long)G : 2048L) * F + 8;
  (void)hipGetLastError();
#define LP_BB_R(TT) hipLaunchKernelGGL(lp_blk_bwd_reduce_kernel<TT>, dim3(B, N * G), dim3(256), 0, stream, (const unsigned short*)c2x, (const unsigned short*)dout, (const unsigned short*)res, sp, gamma, beta, mean, rstd, partial, sep, ds, E, L, span, F, G, cg, lddo)
  lp_typed(dtype, [&](auto t) { LP_BB_R(decltype(t)); });
#undef LP_BB_R
  BTS_LAUNCH_CHECK();
  // Between the reduce and the apply pass (review: ~100 launches of 5-10 us on this chain per step): ONE launch for the two finalizes that
  // only need the reduce pass's partials (GroupNorm class sums -> dgamma / dbeta / c1 / c2; gate partials -> per-(n, c) sums), then the
  // per-sample SE-MLP backward (dgap: the apply pass needs it).  The sums over the samples (dW1, dW2, dw_sp) and the two bias-gradient
  // finalizes wait for the tail launch behind the apply pass: nothing on the chain reads them.
  hipLaunchKernelGGL(lp_blk_bwd_middle_kernel, dim3(G + (N * F + 3) / 4), dim3(256), 0, stream, partial, gamma, dgamma, dbeta, c1, c2, sep, red, N, G, B, cg,
                     (double)L, G * B, F);
  BTS_LAUNCH_CHECK();
  const int r = bts_se_mlp_bwd_sample_(red, scratch, h, ch, w1, w2, dgap, N, V, F, R, stream);
  if (r != BTS_OK) return r;
  int Ba;
  const long per = lp_chunk_per(L, (long)N * G, &Ba, 2048);
  const long blocks = (long)N * G * Ba;
#define LP_BB_A(TT) hipLaunchKernelGGL(lp_blk_bwd_apply_kernel<TT>, dim3((unsigned)Ba, (unsigned)(N * G)), dim3(256), 0, stream, (const unsigned short*)c2x, (const unsigned short*)dout, (unsigned short*)dc2, (unsigned short*)dres, gamma, beta, mean, rstd, c1, c2, sp, ds, ch, wsp, dgap, L, per, F, G, cg, lddo, dbias_c2 ? dbp1 : (double*)nullptr, dbias_pt ? dbp2 : (double*)nullptr)
  lp_typed(dtype, [&](auto t) { LP_BB_A(decltype(t)); });
#undef LP_BB_A
  BTS_LAUNCH_CHECK();
  const int np = (R * F + 255) / 256;
  hipLaunchKernelGGL(lp_blk_bwd_tail_kernel, dim3(np + (dbias_c2 ? F : 0) + (dbias_pt ? F : 0)), dim3(256), 0, stream, red, gap, h, dw1, dw2, dwsp, scratch,
                     N, F, R, np, dbias_c2 ? dbp1 : (const double*)nullptr, dbias_c2, dbias_pt ? dbp2 : (const double*)nullptr, dbias_pt, (int)blocks);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void lp_se_bwd_apply_kernel(const unsigned short* dout, const float* sp, const float* ds, const float* ch,
                                                              const float* wsp, const float* dgap, unsigned short* dres, long NV, long V, int F,
                                                              int lddo, double* dbias_part) {
  __shared__ float dbsh[256 * 8];
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int F8 = F >> 3;
  const long total = NV * F8;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long v = i / F8;
    const int c = (int)(i - v * F8) * 8;
    const long n = v / V;
    float d[8], o[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(dout + v * lddo + c), d);
    const float s = sp[v], dsv = ds[v];
#pragma unroll
    for (int e = 0; e < 8; ++e) { o[e] = fmaf(d[e], s + ch[n * F + c + e], fmaf(dsv, wsp[c + e], dgap[n * F + c + e])); cs[e] += o[e]; }
    *reinterpret_cast<u32x4*>(dres + v * F + c) = pack8<T>(o);
  }
  if (dbias_part != nullptr)     // (launch-uniform; 256 % (F/8) == 0: thread t always holds octet t mod F/8)
    lp_dbias_block(cs, 0, F8, dbias_part + (long)blockIdx.x * F, dbsh);
}
extern "C" long bts_lp_se_bwd_workspace(int N, long V, int F, int R) {
  if (N <= 0 || V <= 0 || F < 8 || R <= 0) return -1;
  long vspan;
  const int B = lp_se_blocks(V, N, F, &vspan);
  return (long)N * B * F * 2 * 8 + ((long)N * F * 3 + (long)N * R) * 8 + 128 + 16384L * F * 8 + 64;   // (+ bias-gradient rows)
}
// dout rows of stride lddo, res dense, both in the storage type; sp fp32 [N*V] (bts_lp_block_epilogue's sp_out); gap / h / ch from the forward.
// Outputs: dres dense in the storage type, ds [N*V] and dgap [N*F] fp32 scratch, parameter gradients fp32 (+= when accumulate_params).
extern "C" int bts_lp_se_bwd(int dtype, const void* dout, const void* res, const float* sp, const float* gap, const float* h, const float* ch,
                             const float* w1, const float* w2, const float* wsp, void* dres, float* ds, float* dgap, float* dw1, float* dw2,
                             float* dwsp, void* workspace, long workspace_bytes, int N, long V, int F, int R, int lddo, int accumulate_params,
                             float* dbias, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || F < 8 || (F & (F - 1)) || F > 256 || lddo < F || lddo % 8) return BTS_ERR_SHAPE;
  if ((((uintptr_t)dout) & 15) || (((uintptr_t)res) & 15) || (((uintptr_t)dres) & 15)) return BTS_ERR_ALIGN;
  if (workspace_bytes < bts_lp_se_bwd_workspace(N, V, F, R)) return BTS_ERR_WORKSPACE;
  long vspan;
  const int B = lp_se_blocks(V, N, F, &vspan);
  double* partial = reinterpret_cast<double*>(workspace);
  double* red = partial + (long)N * B * F * 2;
  double* scratch = red + (long)N * F * 2;
  double* dbp = dbias ? reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(scratch + (long)N * F + (long)N * R) + 63) & ~(uintptr_t)63) : nullptr;
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_se_bwd_reduce_kernel<decltype(t)>, dim3(B, N), dim3(256), 0, stream, (const unsigned short*)dout, (const unsigned short*)res, sp, ds, partial, V, F, lddo, vspan);
  });
  BTS_LAUNCH_CHECK();
  const int r = bts_se_bwd_middle_(partial, red, scratch, gap, h, ch, w1, w2, dw1, dw2, dwsp, dgap, N, B, V, F, R, accumulate_params, stream);
  if (r != BTS_OK) return r;
  const long total = (long)N * V * (F / 8);
  long blocks = (total + 255) / 256;
  const long cap = dbias ? 2048 : 16384;
  if (blocks > cap) blocks = cap;
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_se_bwd_apply_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, stream, (const unsigned short*)dout, sp, ds, ch, wsp, dgap, (unsigned short*)dres, (long)N * V, V, F, lddo, dbp);
  });
  BTS_LAUNCH_CHECK();
  if (dbias != nullptr) {      // bias gradient of the block's 1x1x1 shortcut conv (dres IS its dy)
    return bts_lp_dbias_finalize_(dbp, dbias, F, (int)blocks, F, accumulate_params, stream);
  }
  return BTS_OK;
}
