// GroupNormalization on 16-bit tensors: statistics and apply of the forward, the backward (reduce, finalize, apply with the producing
// conv's bias gradient), and the entry point that runs conv2's data gradient with GroupNorm-1's backward behind it.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.h"
#include "bts_internal.h"
#include "lowp_common.h"
#include "finalize_parts.h"

// ---- GroupNormalization statistics (group_norm.py:100-107): per (n, group) sum and sum of squares from the STORED values,
// fp64 partials per block, fixed-order combine (bts_gn_finalize_partials_).  Dense tensors (ld == C).
//   slab mode: group g of sample n = elements [g*L, (g+1)*L) of the sample's flattened (D,H,W,C) memory
//   channel mode: group g = channels [g*cg, (g+1)*cg)
template <typename T>
__global__ __launch_bounds__(256) void lp_gn_stats_kernel(const unsigned short* x, double* partial, long E, long L, int C, int G, int cg,
                                                          int mode, int B) {
  __shared__ double sh[8];
  const int unit = blockIdx.y;          // n*G + g
  const int n = unit / G, g = unit % G;
  const unsigned short* base = x + (long)n * E;
  double s = 0.0, q = 0.0;
  if (mode == BTS_GN_SLAB) {
    const long lo = (long)g * L;
    const long per = ((L / 8 + B - 1) / B) * 8;
    const long a = lo + (long)blockIdx.x * per, bnd = (a + per < lo + L) ? a + per : lo + L;
    float fs = 0.f, fq = 0.f;
    long cnt = 0;
    for (long i = a + threadIdx.x * 8L; i < bnd; i += 256 * 8) {
      float v[8];
      unpack8<T>(*reinterpret_cast<const u32x4*>(base + i), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) { fs += v[e]; fq = fmaf(v[e], v[e], fq); }
      if (++cnt == 64) { s += fs; q += fq; fs = fq = 0.f; cnt = 0; }   // bounded fp32 run lengths (512 values per lane)
    }
    s += fs; q += fq;
  } else {
    const long V = E / C;
    const long per = (V + B - 1) / B;
    const long a = (long)blockIdx.x * per, bnd = (a + per < V) ? a + per : V;
    const int c0 = g * cg;
    for (long v = a + threadIdx.x; v < bnd; v += 256) {
      float fs = 0.f, fq = 0.f;
      for (int c = 0; c < cg; ++c) { const float t = T::ld(base[v * C + c0 + c]); fs += t; fq = fmaf(t, t, fq); }
      s += fs; q += fq;
    }
  }
  s = block_sum_f64(s, sh);
  q = block_sum_f64(q, sh + 4);
  if (threadIdx.x == 0) {
    double* o = partial + ((long)unit * B + blockIdx.x) * 2;
    o[0] = s; o[1] = q;
  }
}
static int lp_gn_blocks(long L) {
  long b = L / (256 * 8 * 8);
  if (b < 1) b = 1;
  if (b > 256) b = 256;
  return (int)b;
}
extern "C" long bts_lp_gn_workspace(int N, long V, int C, int G) {
  if (N <= 0 || V <= 0 || C <= 0 || G <= 0 || C % G != 0) return -1;
  return (long)N * G * lp_gn_blocks(V * C / G) * 2 * 8 + 64;
}
extern "C" int bts_lp_gn_stats(int dtype, const void* x, float* mean, float* rstd, void* workspace, long workspace_bytes, int N, long V,
                               int C, int G, int mode, float eps, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || G <= 0 || C < G || C % G != 0) return BTS_ERR_SHAPE;
  const long E = V * C, L = E / G;
  if (mode == BTS_GN_SLAB && (E % G != 0 || L % 8 != 0)) return BTS_ERR_UNSUPPORTED;
  if ((((uintptr_t)x) | ((uintptr_t)workspace)) & 15) return BTS_ERR_ALIGN;
  const int B = lp_gn_blocks(L);
  if (workspace_bytes < bts_lp_gn_workspace(N, V, C, G)) return BTS_ERR_WORKSPACE;
  double* partial = reinterpret_cast<double*>(workspace);
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_gn_stats_kernel<decltype(t)>, dim3(B, N * G), dim3(256), 0, stream, (const unsigned short*)x, partial, E, L, C, G, C / G, mode, B);
  });
  BTS_LAUNCH_CHECK();
  return bts_gn_finalize_partials_(partial, mean, rstd, N * G, B, (double)L, eps, stream);
}

// ---- y = [relu]((x - mean) * rstd * gamma[idx] + beta[idx])  (group_norm.py:110-122); x dense, y rows of stride ldy
template <typename T>
__global__ __launch_bounds__(256) void lp_gn_apply_kernel(const unsigned short* x, unsigned short* y, const float* gamma, const float* beta,
                                                          const float* mean, const float* rstd, long total8, long E, long L, int C, int G,
                                                          int cg, int ldy, int mode, int relu) {
  for (long f = blockIdx.x * 256L + threadIdx.x; f < total8; f += (long)gridDim.x * 256) {
    const long i = f * 8;
    const long n = i / E;
    const long r = i - n * E;
    const int c = (int)(r % C);
    const long pix = i / C;
    float v[8], o[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(x + i), v);
    const int gsl = (int)(r / L);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int g = (mode == BTS_GN_SLAB) ? gsl : (c + e) / cg;
      const int idx = (mode == BTS_GN_SLAB) ? g * cg + ((c + e) % cg) : (c + e);
      float t = (v[e] - mean[n * G + g]) * rstd[n * G + g] * gamma[idx] + beta[idx];
      if (relu) t = fmaxf(t, 0.f);
      o[e] = t;
    }
    *reinterpret_cast<u32x4*>(y + pix * ldy + c) = pack8<T>(o);
  }
}
// The same pass for tensors whose (sample, slab) units are whole multiples of 2048 elements with C | 2048 (every layer of the model):
// a workgroup streams one contiguous chunk of one unit, so a thread's eight channels -- and with them its statistics, scales and
// shifts -- are fixed before the loop: no division and no parameter load per 16 bytes, four loads in flight per thread.  (The
// grid-stride form above spent 4 64-bit divisions + 16 small ones per 16 bytes and streamed 3.1 TB/s; this one is bound by HBM.)
// Chunks of one unit: lp_chunk_per (lowp_common.h).
template <typename T, int RELU>
__global__ __launch_bounds__(256) void lp_gn_apply_chunk_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd, long Lu,
                                                                long per, int C, int G, int cg, int ldy, int slab, int upn) {
  const int unit = blockIdx.y, n = unit / upn, u = unit - n * upn;
  const long lo = (long)unit * Lu;
  const long a = lo + (long)blockIdx.x * per;
  const long bnd = (a + per < lo + Lu) ? a + per : lo + Lu;
  const int t8 = threadIdx.x * 8, c = t8 % C;
  float mu[8], sc[8], be[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int g = slab ? u : (c + e) / cg;
    const int idx = slab ? g * cg + ((c + e) % cg) : (c + e);
    mu[e] = mean[n * G + g];
    sc[e] = rstd[n * G + g] * gamma[idx];
    be[e] = beta[idx];
  }
  const long pstep = 2048 / C;
  long pix = a / C + t8 / C;
  const unsigned short* src = x + a + t8;
  const long K = (bnd - a) / 2048;
  auto one = [&](const u32x4 raw, long px) {
    float v[8], o[8];
    unpack8<T>(raw, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = fmaf(v[e] - mu[e], sc[e], be[e]);
      o[e] = RELU ? fmaxf(t, 0.f) : t;
    }
    *reinterpret_cast<u32x4*>(y + px * ldy + c) = pack8<T>(o);
  };
  long k = 0;
  for (; k + 4 <= K; k += 4) {
    u32x4 r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = *reinterpret_cast<const u32x4*>(src + (k + j) * 2048);
#pragma unroll
    for (int j = 0; j < 4; ++j) one(r[j], pix + (k + j) * pstep);
  }
  for (; k < K; ++k) one(*reinterpret_cast<const u32x4*>(src + k * 2048), pix + k * pstep);
}
extern "C" int bts_lp_gn_apply(int dtype, const void* x, void* y, const float* gamma, const float* beta, const float* mean,
                               const float* rstd, int N, long V, int C, int ldy, int G, int mode, int relu, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || C <= 0 || G <= 0 || C < G || C % G != 0 || C % 8 != 0 || ldy % 8 != 0 || ldy < C) return BTS_ERR_SHAPE;
  const long E = V * C, L = E / G;
  if (mode == BTS_GN_SLAB && L % 8 != 0) return BTS_ERR_UNSUPPORTED;
  if ((((uintptr_t)x) & 15) || (((uintptr_t)y) & 15)) return BTS_ERR_ALIGN;
  (void)hipGetLastError();
  {
    const int slab = mode == BTS_GN_SLAB;
    const long Lu = slab ? L : E;
    if (2048 % C == 0 && Lu % 2048 == 0) {
      const int upn = slab ? G : 1;
      int B;
      const long per = lp_chunk_per(Lu, (long)N * upn, &B);
      const dim3 grid((unsigned)B, (unsigned)(N * upn));
#define LP_GA(T_, R_) hipLaunchKernelGGL((lp_gn_apply_chunk_kernel<T_, R_>), grid, dim3(256), 0, stream, (const unsigned short*)x, (unsigned short*)y, gamma, beta, mean, rstd, Lu, per, C, G, C / G, ldy, slab, upn)
      lp_typed(dtype, [&](auto t) {
        using T = decltype(t);
        if (relu) LP_GA(T, 1); else LP_GA(T, 0);
      });
#undef LP_GA
      BTS_LAUNCH_CHECK();
      return BTS_OK;
    }
  }
  const long total8 = (long)N * E / 8;
  long blocks = (total8 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_gn_apply_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, stream, (const unsigned short*)x, (unsigned short*)y, gamma, beta, mean, rstd, total8, E, L, C, G, C / G, ldy, mode, relu);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// =====================================================================================================================
// GroupNormalization backward on 16-bit tensors (channels_last = slab semantics; group_norm.py:83-124 under TF autodiff).
// With xh = (x - mean) * rstd, y = gamma_i xh + beta_i (i = g*cg + c mod cg), dyE = dy * [y > 0] (fused ReLU):
//   A_j = sum dyE * xh, B_j = sum dyE per (n, g, j = c mod cg)   ->  dgamma_i (+)= sum_n A_j, dbeta_i (+)= sum_n B_j
//   c1 = sum_j gamma_j B_j / L,  c2 = sum_j gamma_j A_j / L       ->  dx = (dyE gamma_i - c1 - xh c2) * rstd
// Sums in fp32 runs flushed to fp64, fixed order; dx is written in the storage type (for the data-gradient convs) AND, when
// asked, in fp32 (the weight-gradient kernels still run on the fp32 matrix pipe): one pass instead of three.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void lp_gn_bwd_reduce_kernel(const unsigned short* x, const unsigned short* dy, const float* gamma,
                                                               const float* beta, const float* mean, const float* rstd, double* partial,
                                                               long E, long L, long span, int C, int G, int cg, int lddy, int relu) {
  __shared__ double sh[4 * 4 * 16];
  const int unit = blockIdx.y, n = unit / G, g = unit % G;
  const long lo = (long)blockIdx.x * span;
  long hi = lo + span;
  if (hi > L) hi = L;
  const long ubase = (long)g * L;
  const int cph = (int)((ubase + lo + threadIdx.x * 8L) % C);   // constant over the loop: the stride 2048 is a multiple of C
  float gam[8], bet[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { const int idx = g * cg + ((cph + e) % cg); gam[e] = gamma[idx]; bet[e] = beta[idx]; }
  const float m = mean[unit], rs = rstd[unit];
  double a[8], b[8];
  float fa[8], fb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] = b[e] = 0.0; fa[e] = fb[e] = 0.f; }
  const unsigned short* xb = x + (long)n * E + ubase;
  const long pstep = 2048 / C, pix0 = ((long)n * E + ubase + lo + threadIdx.x * 8L) / C;
  int cnt = 0;
  for (long i = lo + threadIdx.x * 8L; i < hi; i += 2048) {
    float v[8], d[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(xb + i), v);
    const long pix = pix0 + (i - lo) / 2048 * pstep;      // (voxel of the possibly strided dy; 2048 / C voxels per step)
    unpack8<T>(*reinterpret_cast<const u32x4*>(dy + pix * lddy + cph), d);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (v[e] - m) * rs;
      float de = d[e];
      if (relu && !(xh * gam[e] + bet[e] > 0.f)) de = 0.f;
      fa[e] = fmaf(de, xh, fa[e]);
      fb[e] += de;
    }
    if (++cnt == 32) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] += fa[e]; b[e] += fb[e]; fa[e] = fb[e] = 0.f; }
      cnt = 0;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { a[e] += fa[e]; b[e] += fb[e]; }
  // lanes whose 8 channels fall on the same classes: every p-th lane, p = cg / 8 (1 when cg <= 8)
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
    const int cph0 = (int)((ubase + lo) % C);          // lane q of any wave has channel phase cph0 + 8q (+ wave * 512: a multiple of C)
    double sa = 0.0, sb = 0.0;
    for (int w = 0; w < 4; ++w)
      for (int q = 0; q < p; ++q)
        for (int e = 0; e < 8; ++e)
          if (((cph0 + 8 * q + e) % cg) == j) { sa += sh[((w * 4 + q) * 8 + e) * 2]; sb += sh[((w * 4 + q) * 8 + e) * 2 + 1]; }
    double* o = partial + (((long)unit * gridDim.x + blockIdx.x) * cg + j) * 2;
    o[0] = sa; o[1] = sb;
  }
}
__global__ __launch_bounds__(256) void lp_gn_bwd_finalize_kernel(const double* partial, const float* gamma, float* dgamma, float* dbeta, float* c1,
                                                                 float* c2, int N, int G, int B, int cg, double L, int accum) {
  __shared__ double sh[256 * 2];
  __shared__ double tot[256 * 2];
  lp_gn_bwd_finalize_body(partial, gamma, dgamma, dbeta, c1, c2, N, G, B, cg, L, accum, blockIdx.x, sh, tot);
}
// apply pass, chunked like lp_gn_apply_chunk_kernel: a workgroup streams one contiguous piece of one (n, group) unit, a thread's
// channels / statistics / c1, c2 are loop constants (the grid-stride form did 5 64-bit divisions per 16 bytes: 3.9 TB/s)
template <typename T>
__global__ __launch_bounds__(256) void lp_gn_bwd_apply_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
                                                              unsigned short* __restrict__ dx, float* __restrict__ dx32,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ c1, const float* __restrict__ c2, long L, long per, int C,
                                                              int G, int cg, int lddy, int relu, double* dbias_part) {
  __shared__ float dbsh[256 * 8];
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int unit = blockIdx.y, g = unit % G;
  const long lo = (long)unit * L;                      // (= n * E + g * L)
  const long a = lo + (long)blockIdx.x * per;
  const long bnd = (a + per < lo + L) ? a + per : lo + L;
  const int t8 = threadIdx.x * 8, c = t8 % C;
  float gam[8], bet[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { const int idx = g * cg + ((c + e) % cg); gam[e] = gamma[idx]; bet[e] = beta[idx]; }
  const float m = mean[unit], rs = rstd[unit], k1 = c1[unit], k2 = c2[unit];
  const long pstep = 2048 / C, pix = a / C + t8 / C;
  const long K = (bnd - a) / 2048;
  auto one = [&](const u32x4 rx, const u32x4 rd, long i) {
    float v[8], d[8], o[8];
    unpack8<T>(rx, v);
    unpack8<T>(rd, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (v[e] - m) * rs;
      float de = d[e];
      if (relu && !(xh * gam[e] + bet[e] > 0.f)) de = 0.f;
      o[e] = (de * gam[e] - k1 - xh * k2) * rs;
      cs[e] += o[e];
    }
    *reinterpret_cast<u32x4*>(dx + i) = pack8<T>(o);
    if (dx32 != nullptr) {
      *reinterpret_cast<f32x4*>(dx32 + i) = f32x4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<f32x4*>(dx32 + i + 4) = f32x4{o[4], o[5], o[6], o[7]};
    }
  };
  long k = 0;
  for (; k + 2 <= K; k += 2) {
    u32x4 rx[2], rd[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      rx[j] = *reinterpret_cast<const u32x4*>(x + a + t8 + (k + j) * 2048);
      rd[j] = *reinterpret_cast<const u32x4*>(dy + (pix + (k + j) * pstep) * lddy + c);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) one(rx[j], rd[j], a + t8 + (k + j) * 2048);
  }
  for (; k < K; ++k)
    one(*reinterpret_cast<const u32x4*>(x + a + t8 + k * 2048), *reinterpret_cast<const u32x4*>(dy + (pix + k * pstep) * lddy + c), a + t8 + k * 2048);
  if (dbias_part != nullptr)     // (launch-uniform; 2048 % C == 0: thread t always holds octet t mod C/8)
    lp_dbias_block(cs, 0, C / 8, dbias_part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * C, dbsh);
}
extern "C" long bts_lp_gn_bwd_workspace(int N, long V, int C, int G) {
  if (N <= 0 || V <= 0 || C <= 0 || G <= 0 || C % G != 0) return -1;
  const long L = V * C / G;
  return (long)N * G * lp_gnb_blocks(L) * (C / G) * 2 * 8 + (long)N * G * 2 * 4 + 64 + 16384L * C * 8 + 64;   // (+ bias-gradient rows)
}
// x dense (N,V,C) in the storage type; dy rows of stride lddy; dx dense in the storage type, dx32 (may be NULL) the same values in fp32
// finalize + apply (+ bias-gradient finalize) on class-sum partial rows [N*G][B][cg][2] -- lp_gn_bwd_reduce_kernel's, or the ones a
// data-gradient conv left from its epilogue (LpGnbFuse).  tail: c1, c2 ([N*G] floats each), then the 64-byte aligned bias rows
static int lp_gn_bwd_tail(int dtype, const void* x, const void* dy, void* dx, float* dx32, const float* gamma, const float* beta, const float* mean,
                          const float* rstd, float* dgamma, float* dbeta, const double* partial, int B, float* tail, int N, long L, int C, int lddy,
                          int G, int relu, int accumulate_params, float* dbias, hipStream_t stream) {
  const int cg = C / G;
  float* c1 = tail;
  float* c2 = c1 + (long)N * G;
  double* dbp = dbias ? reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(c2 + (long)N * G) + 63) & ~(uintptr_t)63) : nullptr;
  hipLaunchKernelGGL(lp_gn_bwd_finalize_kernel, dim3(G), dim3(256), 0, stream, partial, gamma, dgamma, dbeta, c1, c2, N, G, B, cg, (double)L, accumulate_params);
  BTS_LAUNCH_CHECK();
  int Ba;
  const long per = lp_chunk_per(L, (long)N * G, &Ba, dbias ? 2048 : 4096);   // (bias rows: one per block -- 2048 blocks of 256 fill the chip eight waves deep)
  const long blocks = (long)N * G * Ba;
  if (blocks > 16384) return BTS_ERR_SHAPE;       // (the bias rows of the workspace)
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_gn_bwd_apply_kernel<decltype(t)>, dim3((unsigned)Ba, (unsigned)(N * G)), dim3(256), 0, stream, (const unsigned short*)x, (const unsigned short*)dy, (unsigned short*)dx, dx32, gamma, beta, mean, rstd, c1, c2, L, per, C, G, cg, lddy, relu, dbp);
  });
  BTS_LAUNCH_CHECK();
  if (dbias != nullptr) {      // bias gradient of the conv whose output this GroupNorm normalised (dx IS that conv's dy)
    return bts_lp_dbias_finalize_(dbp, dbias, C, (int)blocks, C, accumulate_params, stream);
  }
  return BTS_OK;
}
static int lp_gn_bwd_check(int dtype, const void* x, const void* dy, const void* dx, const float* dx32, int N, long V, int C, int lddy, int G) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || G <= 0 || C < G || C % G != 0 || C % 8 != 0 || C > 256 || (C & (C - 1)) != 0 || lddy % 8 != 0 || lddy < C) return BTS_ERR_SHAPE;
  if (!lp_gn_bwd_tiled(V, C, G)) return BTS_ERR_UNSUPPORTED;   // (the caller falls back to the fp32 kernels)
  if ((((uintptr_t)x) & 15) || (((uintptr_t)dy) & 15) || (((uintptr_t)dx) & 15) || (dx32 && (((uintptr_t)dx32) & 15))) return BTS_ERR_ALIGN;
  return BTS_OK;
}
extern "C" int bts_lp_gn_bwd_tiled(long V, int C, int G) { return lp_gn_bwd_tiled(V, C, G) ? 1 : 0; }
extern "C" int bts_lp_gn_bwd(int dtype, const void* x, const void* dy, void* dx, float* dx32, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, float* dgamma, float* dbeta, void* workspace, long workspace_bytes, int N,
                             long V, int C, int lddy, int G, int relu, int accumulate_params, float* dbias, hipStream_t stream) {
  const int chk = lp_gn_bwd_check(dtype, x, dy, dx, dx32, N, V, C, lddy, G);
  if (chk != BTS_OK) return chk;
  const long E = V * C, L = E / G;
  const int cg = C / G;
  if (workspace_bytes < bts_lp_gn_bwd_workspace(N, V, C, G)) return BTS_ERR_WORKSPACE;
  const int B = lp_gnb_blocks(L);
  const long span = ((L / 2048 + B - 1) / B) * 2048;
  double* partial = reinterpret_cast<double*>(workspace);
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_gn_bwd_reduce_kernel<decltype(t)>, dim3(B, N * G), dim3(256), 0, stream, (const unsigned short*)x, (const unsigned short*)dy, gamma, beta, mean, rstd, partial, E, L, span, C, G, cg, lddy, relu);
  });
  BTS_LAUNCH_CHECK();
  return lp_gn_bwd_tail(dtype, x, dy, dx, dx32, gamma, beta, mean, rstd, dgamma, dbeta, partial, B, reinterpret_cast<float*>(partial + (long)N * G * B * cg * 2),
                        N, L, C, lddy, G, relu, accumulate_params, dbias, stream);
}

// da = conv3x3x3^T(dy) (stride 1; stored dense in the storage type) and the backward of the GroupNormalization (+ReLU) that da is the
// output gradient of -- resnet.py:80-93 in reverse under train.py:151: conv2's data gradient, then norm1 -- as ONE entry point, so that
// the class sums GroupNorm's backward needs first (A_j, B_j above) leave the conv's epilogue instead of costing a reduce pass over da
// and c (2 of the 5 tensor passes of a GroupNorm backward).  Fused where the z-marching kernel takes the layer (lowp_s1z.hip: the
// data-gradient contraction over 16 | 32 channels, <= 32 GroupNorm channels, whole planes per group); otherwise the conv and
// bts_lp_gn_bwd run back to back: same results up to the order of the fp32 class sums.  (D,H,W): the grid; Cg = GroupNorm channels =
// the forward conv's INPUT channels, Cdy = dy's channels (row stride lddy); wp_bwd = bts_lp_pack(BTS_CONV_K3S1, BTS_ROLE_BWD_DATA, ...).
// *fused_out (may be NULL) <- 1 when the epilogue form ran, 0 otherwise.
static long lp_bwd_data_gn_bwd_workspace(int N, int D, int H, int W, int Cg, int Cdy, int G, LpS1Choice& ch) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cg <= 0 || Cdy <= 0 || G <= 0 || Cg % G != 0) return -1;
  LpS1Call c = lp_s1_call(N, D, H, W, Cdy, Cg);
  c.gnb_G = G;
  lp_s1_choose(c, ch);
  const long conv = ((ch.ws + 63) / 64) * 64;
  const long plain = bts_lp_gn_bwd_workspace(N, (long)D * H * W, Cg, G);
  const long B = ch.B;
  const long fused = B > 0 ? (long)N * G * B * (Cg / G) * 2 * 8 + (long)N * G * 2 * 4 + 64 + 16384L * Cg * 8 + 64 : 0;
  return conv + (fused > plain ? fused : plain) + 64;
}
extern "C" long bts_lp_conv3d_bwd_data_gn_bwd_workspace(int N, int D, int H, int W, int Cg, int Cdy, int G) {
  LpS1Choice ch;
  return lp_bwd_data_gn_bwd_workspace(N, D, H, W, Cg, Cdy, G, ch);
}
extern "C" int bts_lp_conv3d_bwd_data_gn_bwd(int dtype, const void* dy, const void* wp_bwd, void* da, const void* c, void* dc, float* dc32,
                                             const float* gamma, const float* beta, const float* mean, const float* rstd, float* dgamma,
                                             float* dbeta, void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cg, int Cdy,
                                             int lddy, int G, int relu, int accumulate_params, float* dbias, int* fused_out,
                                             hipStream_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cg <= 0 || Cdy <= 0 || G <= 0 || Cg % G != 0) return BTS_ERR_SHAPE;
  const long V = (long)D * H * W;
  int r = lp_gn_bwd_check(dtype, c, da, dc, dc32, N, V, Cg, Cg, G);
  if (r != BTS_OK) return r;
  LpS1Choice sized, ch;
  if (workspace == nullptr || workspace_bytes < lp_bwd_data_gn_bwd_workspace(N, D, H, W, Cg, Cdy, G, sized) || (((uintptr_t)workspace) & 15))
    return BTS_ERR_WORKSPACE;
  const long conv_ws = ((sized.ws + 63) / 64) * 64;
  char* tail = reinterpret_cast<char*>(workspace) + conv_ws;
  const long L = V * Cg / G;
  const int cg = Cg / G;
  if (fused_out) *fused_out = 0;
  r = lp_conv_check(dtype, dy, wp_bwd, da, N, D, H, W, Cdy, lddy, Cg, Cg);
  if (r != BTS_OK) return r;
  LpS1Call cl = lp_s1_call(N, D, H, W, Cdy, Cg);
  cl.ldx = lddy; cl.gnb_G = G; cl.aligned = lp_al16(dy) && lp_al16(da) && lp_al16(wp_bwd) && lp_al16(c);
  r = lp_s1_choose(cl, ch);
  if (r != BTS_OK) return r;
  LpS1Ptrs q{dy, wp_bwd, nullptr, da, workspace, conv_ws};
  const long B = ch.B;
  if (B > 0 && B <= 0x7fffffffL && lp_s1_same(ch, sized)) {     // (the workspace was sized for dense dy)
    LpGnbFuse f;
    f.x = (const unsigned short*)c; f.gamma = gamma; f.beta = beta; f.mean = mean; f.rstd = rstd;
    f.part = reinterpret_cast<double*>(tail); f.G = G; f.cg = cg; f.relu = relu; f.B = B;
    q.gb = &f;
    r = lp_s1_run(dtype, cl, ch, q, stream);
    if (r != BTS_OK) return r;
    if (fused_out) *fused_out = 1;
    return lp_gn_bwd_tail(dtype, c, da, dc, dc32, gamma, beta, mean, rstd, dgamma, dbeta, f.part, (int)B,
                          reinterpret_cast<float*>(f.part + (long)N * G * B * cg * 2), N, L, Cg, Cg, G, relu, accumulate_params, dbias, stream);
  }
  r = lp_s1_run(dtype, cl, ch, q, stream);
  if (r != BTS_OK) return r;
  return bts_lp_gn_bwd(dtype, c, da, dc, dc32, gamma, beta, mean, rstd, dgamma, dbeta, tail, workspace_bytes - conv_ws, N, V, Cg, Cg, G, relu,
                       accumulate_params, dbias, stream);
}
