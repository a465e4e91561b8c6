// GroupNormalization (+ fused ReLU) forward and backward, HBM-bound streaming kernels for gfx950.
// Reference: layers/group_norm.py:83-124 (call), :42-81 (build). Two semantics:
//   BTS_GN_SLAB    channels_last path: the raw reshape [N,D,H,W,C]->[N,G,D,H,W,C/G] makes group g the g-th
//                  contiguous 1/G chunk of each sample's flattened (D,H,W,C) memory; affine index for an
//                  element with channel c is g*(C/G) + (c mod C/G)   (group_norm.py:93-100,115-120)
//   BTS_GN_CHANNEL channels_first path: textbook GroupNorm, affine index = c
// Statistics: population variance, eps inside the sqrt (group_norm.py:105-107). Sums are carried in fp64
// (short fp32 runs per lane, fp64 across lanes/blocks) and combined in a fixed order, so results are
// reproducible run to run; no float atomics.
// x is always a dense NDHWC tensor (ld == C: the raw conv output); y / dy may be channel slices (ld >= C).
#include <stdlib.h>
#include "common.h"
#include "bts_internal.h"
#include "finalize_parts.h"

#define GN_BLOCKS_MAX 256

struct GnGeom {
  int N, C, G, cg, mode;
  long V;      // voxels per sample
  long E;      // elements per sample = V*C
  long L;      // elements per group = E/G
  int B;       // blocks per reduction unit (slab: per (n,g); channel: per n)
  long span;   // elements per block (multiple of 1024)
  int generic; // 1: shape outside the vectorised fast path (C or L not a multiple of 4, C not a power of two)
};

static int gn_geom(GnGeom& g, int N, long V, int C, int G, int mode) {
  if (N <= 0 || V <= 0 || C <= 0 || G <= 0) return BTS_ERR_SHAPE;
  if (C < G || C % G != 0) return BTS_ERR_SHAPE;  // group_norm.py:51-59 (ValueError at the Python layer)
  g.N = N; g.C = C; g.G = G; g.cg = C / G; g.mode = mode; g.V = V; g.E = V * C; g.L = g.E / G;
  if (g.E % G != 0) return BTS_ERR_UNSUPPORTED;
  g.generic = (C % 4 != 0 || (C & (C - 1)) != 0 || C > 1024 || g.L % 4 != 0) ? 1 : 0;
  const long unit = (mode == BTS_GN_SLAB) ? g.L : g.E;
  const int units = (mode == BTS_GN_SLAB) ? N * G : N;
  long B = (2048 + units - 1) / units;  // aim for ~2048 blocks in flight
  if (B > GN_BLOCKS_MAX) B = GN_BLOCKS_MAX;
  long span = (unit + B - 1) / B;
  span = (span + 1023) / 1024 * 1024;
  g.span = span;
  g.B = (int)((unit + span - 1) / span);
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// forward statistics
// ---------------------------------------------------------------------------------------------
// slab: grid (B, N*G). partial[(ng*B + b)*2 + {0,1}] = (sum x, sum x^2)
__global__ __launch_bounds__(256) void gn_stats_slab_kernel(const float* __restrict__ x, double* partial, long L, long span) {
  __shared__ double sh[8];
  const long base = (long)blockIdx.y * L;
  const long lo = (long)blockIdx.x * span;
  long hi = lo + span;
  if (hi > L) hi = L;
  double s = 0.0, ss = 0.0;
  for (long i = lo + threadIdx.x * 4; i < hi; i += 1024) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + base + i);
    const float a = (v[0] + v[1]) + (v[2] + v[3]);
    const float b = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    s += (double)a;
    ss += (double)b;
  }
  const double rs = block_sum_f64(s, sh);
  const double rss = block_sum_f64(ss, sh + 4);
  if (threadIdx.x == 0) {
    const long o = ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    partial[o] = rs;
    partial[o + 1] = rss;
  }
}

// channel: grid (B, N). partial[((n*B + b)*C + c)*2 + {0,1}] per channel
__global__ __launch_bounds__(256) void gn_stats_channel_kernel(const float* __restrict__ x, double* partial, long E, long span, int C) {
  __shared__ double sh[256 * 8];
  const long base = (long)blockIdx.y * E;
  const long lo = (long)blockIdx.x * span;
  long hi = lo + span;
  if (hi > E) hi = E;
  double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
  for (long i = lo + threadIdx.x * 4; i < hi; i += 1024) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + base + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] += (double)v[e]; ss[e] += (double)v[e] * (double)v[e]; }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { sh[threadIdx.x * 8 + e] = s[e]; sh[threadIdx.x * 8 + 4 + e] = ss[e]; }
  __syncthreads();
  const int P4 = C / 4;  // threads with equal (tid % P4) hold the same 4 channels (1024 % C == 0)
  for (int c = threadIdx.x; c < C; c += 256) {
    const int e = c & 3, r = c >> 2;
    double a = 0.0, b = 0.0;
    if (P4 <= 256)
      for (int k = r; k < 256; k += P4) { a += sh[k * 8 + e]; b += sh[k * 8 + 4 + e]; }
    const long o = (((long)blockIdx.y * gridDim.x + blockIdx.x) * C + c) * 2;
    partial[o] = a;
    partial[o + 1] = b;
  }
}

// one wave per (n,g): lanes split the partial blocks, fixed-order shuffle tree
__global__ __launch_bounds__(256) void gn_stats_finalize_kernel(const double* partial, float* mean, float* rstd, int NG, int B,
                                                                int C, int G, int mode, double count, float eps) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= NG) return;
  double s = 0.0, ss = 0.0;
  if (mode == BTS_GN_SLAB) {
    for (int b = lane; b < B; b += 64) { s += partial[((long)i * B + b) * 2]; ss += partial[((long)i * B + b) * 2 + 1]; }
  } else {
    const int n = i / G, g = i % G, cg = C / G;
    for (int k = lane; k < B * cg; k += 64) {
      const int b = k / cg, c = g * cg + k % cg;
      const long o = (((long)n * B + b) * C + c) * 2;
      s += partial[o];
      ss += partial[o + 1];
    }
  }
  s = wave_sum_f64(s);
  ss = wave_sum_f64(ss);
  if (lane == 0) {
    const double m = s / count;
    double var = ss / count - m * m;
    if (var < 0.0) var = 0.0;
    mean[i] = (float)m;
    rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
  }
}


// ---------------------------------------------------------------------------------------------
// generic (any C, any L) path: one workgroup per (n,g); used only for shapes the vectorised path rejects
// (tiny test configurations, e.g. 2-channel GroupNorm). Same math, same fixed-order fp64 sums.
// element e of group (n,g): slab -> sample offset g*L + e ; channel -> voxel e/cg, channel g*cg + e%cg
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ long gn_elem_offset(long e, int g, long L, int C, int cg, int mode) {
  return (mode == BTS_GN_SLAB) ? (long)g * L + e : (e / cg) * C + (long)g * cg + (e % cg);
}
__global__ __launch_bounds__(256) void gn_stats_generic_kernel(const float* x, float* mean, float* rstd, long E, long L, int C,
                                                               int G, int cg, int mode, float eps) {
  __shared__ double sh[8];
  const int n = blockIdx.x / G, g = blockIdx.x % G;
  double s = 0.0, ss = 0.0;
  for (long e = threadIdx.x; e < L; e += blockDim.x) {
    const double v = (double)x[(long)n * E + gn_elem_offset(e, g, L, C, cg, mode)];
    s += v; ss += v * v;
  }
  const double rs = block_sum_f64(s, sh);
  const double rss = block_sum_f64(ss, sh + 4);
  if (threadIdx.x == 0) {
    const double m = rs / (double)L;
    double var = rss / (double)L - m * m;
    if (var < 0.0) var = 0.0;
    mean[blockIdx.x] = (float)m;
    rstd[blockIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
  }
}
__global__ void gn_apply_generic_kernel(const float* x, float* y, const float* gamma, const float* beta, const float* mean,
                                        const float* rstd, long total, long E, long L, int C, int G, int cg, int ldy,
                                        int mode, int relu) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / E, r = i - n * E;
    const int c = (int)(r % C);
    const int g = (mode == BTS_GN_SLAB) ? (int)(r / L) : c / cg;
    const int idx = (mode == BTS_GN_SLAB) ? g * cg + (c % cg) : c;
    float o = (x[i] - mean[n * G + g]) * rstd[n * G + g] * gamma[idx] + beta[idx];
    if (relu) o = fmaxf(o, 0.f);
    y[(i / C) * ldy + c] = o;
  }
}
// per (n,g): c1 = sum(dyE*gamma)/L, c2 = sum(dyE*gamma*xh)/L
__global__ __launch_bounds__(256) void gn_bwd_group_generic_kernel(const float* x, const float* dy, const float* gamma,
                                                                   const float* beta, const float* mean, const float* rstd,
                                                                   float* c1, float* c2, long E, long L, int C, int G, int cg,
                                                                   int lddy, int mode, int relu) {
  __shared__ double sh[8];
  const int n = blockIdx.x / G, g = blockIdx.x % G;
  const float m = mean[blockIdx.x], rs = rstd[blockIdx.x];
  double s1 = 0.0, s2 = 0.0;
  for (long e = threadIdx.x; e < L; e += blockDim.x) {
    const long r = gn_elem_offset(e, g, L, C, cg, mode);
    const int c = (int)(r % C);
    const int idx = (mode == BTS_GN_SLAB) ? g * cg + (c % cg) : c;
    const float xh = (x[(long)n * E + r] - m) * rs;
    float de = dy[((long)n * (E / C) + r / C) * lddy + c];
    if (relu && !(xh * gamma[idx] + beta[idx] > 0.f)) de = 0.f;
    // gamma_j B_j and gamma_j A_j as the vectorised route forms them: dE exact, dE * xh rounded once, the products with gamma in fp64
    // (an fp32 dE * gamma put 70 eps32 on a c1 that cancels, visible in dx where dE = 0 and xh ~ 0)
    s1 += (double)de * (double)gamma[idx];
    s2 += (double)(de * xh) * (double)gamma[idx];
  }
  const double r1 = block_sum_f64(s1, sh);
  const double r2 = block_sum_f64(s2, sh + 4);
  if (threadIdx.x == 0) { c1[blockIdx.x] = (float)(r1 / (double)L); c2[blockIdx.x] = (float)(r2 / (double)L); }
}
// per affine index idx: dgamma = sum dyE*xh, dbeta = sum dyE over all samples / elements mapped to idx
__global__ __launch_bounds__(256) void gn_bwd_param_generic_kernel(const float* x, const float* dy, const float* gamma,
                                                                   const float* beta, const float* mean, const float* rstd,
                                                                   float* dgamma, float* dbeta, int N, long E, long L, int C,
                                                                   int G, int cg, int lddy, int mode, int relu, int accum) {
  __shared__ double sh[8];
  const int idx = blockIdx.x;
  const int g = idx / cg, j = idx % cg;
  double sa = 0.0, sb = 0.0;
  for (int n = 0; n < N; ++n)
    for (long e = threadIdx.x; e < L; e += blockDim.x) {
      const long r = gn_elem_offset(e, g, L, C, cg, mode);
      const int c = (int)(r % C);
      if ((c % cg) != j) continue;
      const float xh = (x[(long)n * E + r] - mean[n * G + g]) * rstd[n * G + g];
      float de = dy[((long)n * (E / C) + r / C) * lddy + c];
      if (relu && !(xh * gamma[idx] + beta[idx] > 0.f)) de = 0.f;
      sa += (double)(de * xh);
      sb += (double)de;
    }
  const double ra = block_sum_f64(sa, sh);
  const double rb = block_sum_f64(sb, sh + 4);
  if (threadIdx.x == 0) {
    if (dgamma) dgamma[idx] = accum ? dgamma[idx] + (float)ra : (float)ra;
    if (dbeta) dbeta[idx] = accum ? dbeta[idx] + (float)rb : (float)rb;
  }
}
__global__ void gn_bwd_apply_generic_kernel(const float* x, const float* dy, float* dx, const float* gamma, const float* beta,
                                            const float* mean, const float* rstd, const float* c1, const float* c2, long total,
                                            long E, long L, int C, int G, int cg, int lddy, int mode, int relu) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / E, r = i - n * E;
    const int c = (int)(r % C);
    const int g = (mode == BTS_GN_SLAB) ? (int)(r / L) : c / cg;
    const int idx = (mode == BTS_GN_SLAB) ? g * cg + (c % cg) : c;
    const float rs = rstd[n * G + g];
    const float xh = (x[i] - mean[n * G + g]) * rs;
    float de = dy[(i / C) * lddy + c];
    if (relu && !(xh * gamma[idx] + beta[idx] > 0.f)) de = 0.f;
    dx[i] = (de * gamma[idx] - c1[n * G + g] - xh * c2[n * G + g]) * rs;
  }
}

extern "C" long bts_gn_workspace(int N, long V, int C, int G, int mode) {
  GnGeom g;
  if (gn_geom(g, N, V, C, G, mode) != BTS_OK) return -1;
  // forward: 2 doubles per block (slab) or 2*C per block (channel); backward: 2*C doubles per (n, block-row)
  const long fwd = (mode == BTS_GN_SLAB) ? (long)N * G * g.B * 2 : (long)N * g.B * C * 2;
  const long bwd = (mode == BTS_GN_SLAB) ? (long)N * G * g.B * g.cg * 2 : (long)N * g.B * C * 2;
  return (fwd > bwd ? fwd : bwd) * 8 + 256;
}

extern "C" int bts_gn_stats(const float* x, float* mean, float* rstd, void* workspace, long workspace_bytes, int N,
                            long V, int C, int G, int mode, float eps, hipStream_t stream) {
  GnGeom g;
  int r = gn_geom(g, N, V, C, G, mode);
  if (r != BTS_OK) return r;
  if (workspace == nullptr || workspace_bytes < bts_gn_workspace(N, V, C, G, mode)) return BTS_ERR_WORKSPACE;
  if (g.generic) {
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_stats_generic_kernel, dim3(N * G), dim3(256), 0, stream, x, mean, rstd, g.E, g.L, C, G, g.cg, mode, eps);
    BTS_LAUNCH_CHECK();
    return BTS_OK;
  }
  if (((uintptr_t)x) & 15) return BTS_ERR_ALIGN;
  double* partial = reinterpret_cast<double*>(workspace);
  if (mode == BTS_GN_SLAB) {
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_stats_slab_kernel, dim3(g.B, N * G), dim3(256), 0, stream, x, partial, g.L, g.span);
  } else {
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_stats_channel_kernel, dim3(g.B, N), dim3(256), 0, stream, x, partial, g.E, g.span, C);
  }
  BTS_LAUNCH_CHECK();
  const int NG = N * G;
  (void)hipGetLastError(); hipLaunchKernelGGL(gn_stats_finalize_kernel, dim3((NG + 3) / 4), dim3(256), 0, stream, partial, mean, rstd, NG, g.B,
                     C, G, mode, (double)g.L, eps);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// many partials per unit (conv epilogues leave one per tile column, plane and wave: 5-10 k at 128^3): one 1024-thread WORKGROUP per (n, g),
// fixed order.  Four loads in flight per thread: walking the pairs one by one with 256 threads was a chain of ~40 dependent-latency
// loads, 11 us per launch on the critical path of every GroupNorm.
__global__ __launch_bounds__(1024) void gn_stats_finalize_wide_kernel(const double* partial, float* mean, float* rstd, int B, double count,
                                                                      float eps) {
  __shared__ double sh[32];
  const int i = blockIdx.x;
  double s = 0.0, ss = 0.0;
  const double2* pp = reinterpret_cast<const double2*>(partial) + (long)i * B;
  int b = threadIdx.x;
  for (; b + 3 * 1024 < B; b += 4 * 1024) {
    double2 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = pp[b + j * 1024];
#pragma unroll
    for (int j = 0; j < 4; ++j) { s += v[j].x; ss += v[j].y; }
  }
  for (; b < B; b += 1024) { const double2 v = pp[b]; s += v.x; ss += v.y; }
  s = wave_sum_f64(s);
  ss = wave_sum_f64(ss);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sh[w] = s; sh[16 + w] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double rs = 0.0, rss = 0.0;
    for (int k = 0; k < 16; ++k) { rs += sh[k]; rss += sh[16 + k]; }
    const double m = rs / count;
    double var = rss / count - m * m;
    if (var < 0.0) var = 0.0;
    mean[i] = (float)m;
    rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

int bts_gn_finalize_partials_(const double* partial, float* mean, float* rstd, int NG, long B, double count, float eps,
                              hipStream_t stream) {
  if (NG <= 0 || B <= 0 || B > 0x7fffffffL) return BTS_ERR_SHAPE;
  if (B >= 512) {
    if (((uintptr_t)partial) & 15) return BTS_ERR_ALIGN;     // (only the wide kernel loads double2; the public entry points check their workspace up front)
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_stats_finalize_wide_kernel, dim3(NG), dim3(1024), 0, stream, partial, mean, rstd, (int)B, count, eps);
    BTS_LAUNCH_CHECK();
    return BTS_OK;
  }
  (void)hipGetLastError(); hipLaunchKernelGGL(gn_stats_finalize_kernel, dim3((NG + 3) / 4), dim3(256), 0, stream, partial, mean, rstd, NG, (int)B, 0,
                     1, BTS_GN_SLAB, count, eps);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// forward apply (+ReLU), y may be strided
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       long total4, long E, long L, int C, int G, int cg, int ldy,
                                                       int mode, int relu) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < total4; f += (long)gridDim.x * blockDim.x) {
    const long i = f * 4;
    const long n = i / E;
    const long r = i - n * E;
    const int c = (int)(r % C);
    const long pix = i / C;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
    f32x4 o;
    if (mode == BTS_GN_SLAB) {
      const int g = (int)(r / L);
      const float m = mean[n * G + g], rs = rstd[n * G + g];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = g * cg + ((c + e) % cg);
        o[e] = (v[e] - m) * rs * gamma[idx] + beta[idx];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int g = (c + e) / cg;
        o[e] = (v[e] - mean[n * G + g]) * rstd[n * G + g] * gamma[c + e] + beta[c + e];
      }
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
    }
    *reinterpret_cast<f32x4*>(y + pix * ldy + c) = o;
  }
}

// Slab mode, dense rows (ld == C), L % 1024 == 0: a block owns `cpb` consecutive 1024-element chunks of ONE (n, group) unit, so
// the statistics are block constants and a thread's channel phase (4*tid mod C, 1024 % C == 0) and affine parameters never
// change: the loop is loads, four fused multiply-adds and a store -- no index arithmetic, two chunks in flight.
__global__ __launch_bounds__(256) void gn_apply_slab_stream_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   long chunks_per_unit, int cpb, int C, int cg, int G, int relu, int ldy) {
  const long chunk0 = (long)blockIdx.x * cpb;
  const long unit = chunk0 / chunks_per_unit;          // n*G + g
  const int g = (int)(unit % G);
  const float m = mean[unit], rs = rstd[unit];
  const int c = (threadIdx.x * 4) % C;
  float sc[4], sh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = g * cg + ((c + e) % cg);
    sc[e] = rs * gamma[idx];
    sh[e] = beta[idx];
  }
  const float* xp = x + chunk0 * 1024 + threadIdx.x * 4;
  const long vpc = 1024 / C;   // y may be a channel slice of a wider slab (row stride ldy >= C)
  float* yp = y + (chunk0 * vpc + (threadIdx.x * 4) / C) * ldy + c;
  const long ystep = vpc * ldy;
  int k = 0;
  for (; k + 1 < cpb; k += 2) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(xp + (long)k * 1024);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(xp + (long)(k + 1) * 1024);
    f32x4 o0, o1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o0[e] = fmaf(v0[e] - m, sc[e], sh[e]);   // centred first: no cancellation when |mean| >> std
      o1[e] = fmaf(v1[e] - m, sc[e], sh[e]);
      if (relu) { o0[e] = fmaxf(o0[e], 0.f); o1[e] = fmaxf(o1[e], 0.f); }
    }
    *reinterpret_cast<f32x4*>(yp + (long)k * ystep) = o0;
    *reinterpret_cast<f32x4*>(yp + (long)(k + 1) * ystep) = o1;
  }
  for (; k < cpb; ++k) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(xp + (long)k * 1024);
    f32x4 o0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o0[e] = fmaf(v0[e] - m, sc[e], sh[e]);
      if (relu) o0[e] = fmaxf(o0[e], 0.f);
    }
    *reinterpret_cast<f32x4*>(yp + (long)k * ystep) = o0;
  }
}
// chunks per block for the streaming kernels: the largest power of two <= 8 dividing the chunks of a unit
static int gn_stream_cpb(long chunks_per_unit) {
  int cpb = 8;
  while (cpb > 1 && chunks_per_unit % cpb != 0) cpb >>= 1;
  return cpb;
}

extern "C" int bts_gn_apply(const float* x, float* y, const float* gamma, const float* beta, const float* mean,
                            const float* rstd, int N, long V, int C, int ldy, int G, int mode, int relu,
                            hipStream_t stream) {
  GnGeom g;
  int r = gn_geom(g, N, V, C, G, mode);
  if (r != BTS_OK) return r;
  if (g.generic || ldy % 4 != 0) {
    if (ldy < C) return BTS_ERR_ALIGN;
    const long total = (long)N * g.E;
    int gb = (int)((total + 255) / 256);
    if (gb > 8192) gb = 8192;
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_apply_generic_kernel, dim3(gb), dim3(256), 0, stream, x, y, gamma, beta, mean, rstd, total, g.E, g.L,
                       C, G, g.cg, ldy, mode, relu);
    BTS_LAUNCH_CHECK();
    return BTS_OK;
  }
  if (ldy < C || (((uintptr_t)x) & 15) || (((uintptr_t)y) & 15)) return BTS_ERR_ALIGN;
  if (mode == BTS_GN_SLAB && g.L % 1024 == 0 && 1024 % C == 0) {
    // NOTE: results differ from gn_apply_kernel in the last bit ((x - m) * rs * gamma + beta is evaluated as
    // fma(x - m, rs*gamma, beta)); both are within the element-wise tolerance of the oracle
    const long cpu = g.L / 1024;
    const int cpb = gn_stream_cpb(cpu);
    const long nblk = (long)N * G * cpu / cpb;
    if (nblk <= 0x7fffffffL) {
      (void)hipGetLastError(); hipLaunchKernelGGL(gn_apply_slab_stream_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, x, y, gamma, beta, mean,
                         rstd, cpu, cpb, C, g.cg, G, relu, ldy);
      BTS_LAUNCH_CHECK();
      return BTS_OK;
    }
  }
  const long total4 = (long)N * g.E / 4;
  int blocks = (int)((total4 + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  (void)hipGetLastError(); hipLaunchKernelGGL(gn_apply_kernel, dim3(blocks), dim3(256), 0, stream, x, y, gamma, beta, mean, rstd, total4, g.E,
                     g.L, C, G, g.cg, ldy, mode, relu);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// backward (SURVEY Appendix A'): with xh = (x-mean)*rstd, y = gamma_b*xh + beta_b, dyE = dy * [y>0] (if relu)
//   A_j = sum dyE*xh , B_j = sum dyE  per (n, g, j = c mod cg)      -> dgamma[idx] += sum_n A_j, dbeta likewise
//   c1 = sum_j gamma_j B_j / L , c2 = sum_j gamma_j A_j / L
//   dx = (dyE*gamma_b - c1 - xh*c2) * rstd
// ---------------------------------------------------------------------------------------------
// slab: grid (B, N*G), partial[((ng*B + b)*cg + j)*2 + {A,B}] ; channel: grid (B, N), partial[((n*B+b)*C + c)*2 ..]
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            double* partial, long E, long L, long span, int C, int G,
                                                            int cg, int lddy, int mode, int relu) {
  __shared__ double sh[256 * 8];
  const bool slab = (mode == BTS_GN_SLAB);
  const int n = slab ? blockIdx.y / G : blockIdx.y;
  const int gs = slab ? blockIdx.y % G : 0;
  const long unitBase = slab ? (long)gs * L : 0;  // offset inside the sample
  const long unitLen = slab ? L : E;
  const long lo = (long)blockIdx.x * span;
  long hi = lo + span;
  if (hi > unitLen) hi = unitLen;
  double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
  const long npix = E / C;
  // the channel phase of a thread never changes inside this loop (1024 % C == 0, span % 1024 == 0): fetch its four
  // affine parameters and, in slab mode, the group statistics once
  const int cph = (int)((unitBase + lo + threadIdx.x * 4) % C);
  float gam[4], bet[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = slab ? gs * cg + ((cph + e) % cg) : (cph + e);
    gam[e] = gamma[idx];
    bet[e] = beta[idx];
  }
  const float m_s = mean[n * G + gs], rs_s = rstd[n * G + gs];  // slab mode: the unit's statistics (block constants)
  auto body = [&](const f32x4 v, const f32x4 d, int c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = slab ? gs : (c + e) / cg;
      const float xh = slab ? (v[e] - m_s) * rs_s : (v[e] - mean[n * G + g]) * rstd[n * G + g];
      float de = d[e];
      if (relu && !(xh * gam[e] + bet[e] > 0.f)) de = 0.f;
      a[e] += (double)(de * xh);
      b[e] += (double)de;
    }
  };
  long i = lo + threadIdx.x * 4;
  if (lddy == C) {  // dense dy: it is indexed like x, no division in the loop
    const float* xb = x + (long)n * E + unitBase;
    const float* db = dy + (long)n * E + unitBase;
    for (; i + 3072 < hi; i += 4096) {  // four chunks of both streams in flight
      f32x4 v[4], d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = *reinterpret_cast<const f32x4*>(xb + i + 1024 * u);
        d[u] = *reinterpret_cast<const f32x4*>(db + i + 1024 * u);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) body(v[u], d[u], cph);
    }
    for (; i + 1024 < hi; i += 2048) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(xb + i);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(xb + i + 1024);
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(db + i);
      const f32x4 d1 = *reinterpret_cast<const f32x4*>(db + i + 1024);
      body(v0, d0, cph);
      body(v1, d1, cph);
    }
    for (; i < hi; i += 1024) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xb + i);
      const f32x4 d = *reinterpret_cast<const f32x4*>(db + i);
      body(v, d, cph);
    }
  }
  for (; i + 1024 < hi; i += 2048) {  // two independent 16-B loads per stream in flight
    const long r0 = unitBase + i, r1 = r0 + 1024;
    const int c0 = (int)(r0 % C), c1 = (int)(r1 % C);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + (long)n * E + r0);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(x + (long)n * E + r1);
    const f32x4 d0 = *reinterpret_cast<const f32x4*>(dy + ((long)n * npix + r0 / C) * lddy + c0);
    const f32x4 d1 = *reinterpret_cast<const f32x4*>(dy + ((long)n * npix + r1 / C) * lddy + c1);
    body(v0, d0, c0);
    body(v1, d1, c1);
  }
  for (; i < hi; i += 1024) {
    const long r = unitBase + i;
    const int c = (int)(r % C);
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + (long)n * E + r);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + ((long)n * npix + r / C) * lddy + c);
    body(v, d, c);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { sh[threadIdx.x * 8 + e] = a[e]; sh[threadIdx.x * 8 + 4 + e] = b[e]; }
  __syncthreads();
  // a thread's 4 elements sit at (unitBase + lo + 4*tid + e + 1024*k): channel phase is fixed per thread because
  // 1024 % C == 0, span % 1024 == 0 and (slab) L % cg == 0. Output period P: cg (slab, j = c mod cg) or C (channel).
  const int P = slab ? cg : C;
  for (int j = threadIdx.x; j < P; j += 256) {
    double sa = 0.0, sb = 0.0;
    if (P >= 4) {
      const int e = j & 3, rr = j >> 2, P4 = P >> 2;
      for (int k = rr; k < 256; k += P4) { sa += sh[k * 8 + e]; sb += sh[k * 8 + 4 + e]; }
    } else {  // P == 2 (or 1): elements e with (e % P) == j of every thread
      for (int k = 0; k < 256; ++k)
        for (int e = j; e < 4; e += P) { sa += sh[k * 8 + e]; sb += sh[k * 8 + 4 + e]; }
    }
    const long o = (((long)blockIdx.y * gridDim.x + blockIdx.x) * P + j) * 2;
    partial[o] = sa;
    partial[o + 1] = sb;
  }
}

// stage A: one wave per (n, idx): sum the per-block partials (lanes split the blocks) -> scratch[(n*C+idx)*2 + {A,B}]
__global__ __launch_bounds__(256) void gn_bwd_finalize_a_kernel(const double* partial, double* scratch, int N, int B, int C,
                                                                int G, int mode) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= N * C) return;
  const int cg = C / G;
  const int n = t / C, idx = t % C;
  double sa = 0.0, sb = 0.0;
  if (mode == BTS_GN_SLAB) {
    const int g = idx / cg, j = idx % cg;
    for (int b = lane; b < B; b += 64) {
      const long o = ((((long)n * G + g) * B + b) * cg + j) * 2;
      sa += partial[o];
      sb += partial[o + 1];
    }
  } else {
    for (int b = lane; b < B; b += 64) {
      const long o = (((long)n * B + b) * C + idx) * 2;
      sa += partial[o];
      sb += partial[o + 1];
    }
  }
  sa = wave_sum_f64(sa);
  sb = wave_sum_f64(sb);
  if (lane == 0) { scratch[t * 2] = sa; scratch[t * 2 + 1] = sb; }
}
// stage B (one block): dgamma/dbeta over samples, then c1,c2 per (n,g)
__global__ void gn_bwd_finalize_kernel(const float* gamma, float* dgamma, float* dbeta, float* c1, float* c2,
                                       const double* scratch /*N*C*2*/, int N, int C, int G, double L, int accum) {
  const int cg = C / G;
  for (int idx = threadIdx.x; idx < C; idx += blockDim.x) {
    double sa = 0.0, sb = 0.0;
    for (int n = 0; n < N; ++n) { sa += scratch[(n * C + idx) * 2]; sb += scratch[(n * C + idx) * 2 + 1]; }
    if (dgamma) dgamma[idx] = accum ? dgamma[idx] + (float)sa : (float)sa;
    if (dbeta) dbeta[idx] = accum ? dbeta[idx] + (float)sb : (float)sb;
  }
  for (int t = threadIdx.x; t < N * G; t += blockDim.x) {
    const int n = t / G, g = t % G;
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < cg; ++j) {
      const int idx = g * cg + j;
      s1 += (double)gamma[idx] * scratch[(n * C + idx) * 2 + 1];
      s2 += (double)gamma[idx] * scratch[(n * C + idx) * 2];
    }
    c1[t] = (float)(s1 / L);
    c2[t] = (float)(s2 / L);
  }
}

// slab mode, one launch instead of the two above: one block per group g; threads = (class j, slice of the partial blocks); for every
// sample the class sums over the blocks -> c1, c2; the sums over the samples -> dgamma, dbeta.  (The pair cost two ~4.7 us launches per
// GroupNorm backward on the main stream's chain: 43 of them per step.)  cg = C / G is a power of two <= 256 here.
__global__ __launch_bounds__(256) void gn_bwd_finalize_slab_kernel(const double* partial, const float* gamma, float* dgamma, float* dbeta, float* c1,
                                                                   float* c2, int N, int G, int B, int cg, double L, int accum) {
  __shared__ double sh[256 * 2];
  gn_bwd_finalize_slab_body(partial, gamma, dgamma, dbeta, c1, c2, N, G, B, cg, L, accum, blockIdx.x, sh);
}

__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           float* __restrict__ dx, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ c1,
                                                           const float* __restrict__ c2, long total4, long E, long L,
                                                           int C, int G, int cg, int lddy, int mode, int relu) {
  // grid stride (gridDim*1024 elements) is a multiple of C (power of two <= 1024): a thread's channel phase is fixed,
  // so in channel mode its four affine parameters are loop invariant (slab mode: they also depend on the group)
  const long f0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int cph = (int)((f0 * 4) % C);
  const bool fixed = ((long)gridDim.x * 1024) % C == 0;
  for (long f = f0; f < total4; f += (long)gridDim.x * blockDim.x) {
    const long i = f * 4;
    const long n = i / E;
    const long r = i - n * E;
    const int c = fixed ? cph : (int)(r % C);
    const long pix = i / C;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + pix * lddy + c);
    const int gsl = (int)(r / L);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = (mode == BTS_GN_SLAB) ? gsl : (c + e) / cg;
      const int idx = (mode == BTS_GN_SLAB) ? g * cg + ((c + e) % cg) : (c + e);
      const float rs = rstd[n * G + g];
      const float xh = (v[e] - mean[n * G + g]) * rs;
      float de = d[e];
      const float ga = gamma[idx];
      if (relu && !(xh * ga + beta[idx] > 0.f)) de = 0.f;
      o[e] = (de * ga - c1[n * G + g] - xh * c2[n * G + g]) * rs;
    }
    *reinterpret_cast<f32x4*>(dx + i) = o;
  }
}

// for block_bwd.hip (the fused gate + GroupNorm-2 backward): the slab-mode block geometry of this file
bool bts_gn_slab_blocks_(int N, long V, int C, int G, int* B, long* span) {
  GnGeom g;
  if (gn_geom(g, N, V, C, G, BTS_GN_SLAB) != BTS_OK || g.generic) return false;
  *B = g.B;
  *span = g.span;
  return true;
}
// streaming form of gn_bwd_apply_kernel for slab mode with dense dy (see gn_apply_slab_stream_kernel); same arithmetic, element
// for element, as the general kernel
__global__ __launch_bounds__(256) void gn_bwd_apply_slab_stream_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                       float* __restrict__ dx, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, const float* __restrict__ mean,
                                                                       const float* __restrict__ rstd, const float* __restrict__ c1,
                                                                       const float* __restrict__ c2, long chunks_per_unit, int cpb,
                                                                       int C, int cg, int G, int relu, int lddy) {
  const long chunk0 = (long)blockIdx.x * cpb;
  const long unit = chunk0 / chunks_per_unit;
  const int g = (int)(unit % G);
  const float m = mean[unit], rs = rstd[unit], k1 = c1[unit], k2 = c2[unit];
  const int c = (threadIdx.x * 4) % C;
  float ga[4], be[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = g * cg + ((c + e) % cg);
    ga[e] = gamma[idx];
    be[e] = beta[idx];
  }
  const long off = chunk0 * 1024 + threadIdx.x * 4;
  // dy may be a channel slice of a wider slab (row stride lddy >= C): its rows advance by 1024 / C voxels per chunk
  const long vpc = 1024 / C;
  const long doff = (chunk0 * vpc + (threadIdx.x * 4) / C) * lddy + c;
  const long dstep = vpc * lddy;
  auto one = [&](const f32x4 v, const f32x4 d) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (v[e] - m) * rs;
      float de = d[e];
      if (relu && !(xh * ga[e] + be[e] > 0.f)) de = 0.f;
      o[e] = (de * ga[e] - k1 - xh * k2) * rs;
    }
    return o;
  };
  int k = 0;
  for (; k + 1 < cpb; k += 2) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + off + (long)k * 1024);
    const f32x4 d0 = *reinterpret_cast<const f32x4*>(dy + doff + (long)k * dstep);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(x + off + (long)(k + 1) * 1024);
    const f32x4 d1 = *reinterpret_cast<const f32x4*>(dy + doff + (long)(k + 1) * dstep);
    *reinterpret_cast<f32x4*>(dx + off + (long)k * 1024) = one(v0, d0);
    *reinterpret_cast<f32x4*>(dx + off + (long)(k + 1) * 1024) = one(v1, d1);
  }
  for (; k < cpb; ++k) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + off + (long)k * 1024);
    const f32x4 d0 = *reinterpret_cast<const f32x4*>(dy + doff + (long)k * dstep);
    *reinterpret_cast<f32x4*>(dx + off + (long)k * 1024) = one(v0, d0);
  }
}

// gn backward: dx dense (ld == C). small_ws: >= (N*G*2 floats + N*C*2 doubles) scratch inside workspace tail.
extern "C" int bts_gn_bwd(const float* x, const float* dy, float* dx, const float* gamma, const float* beta,
                          const float* mean, const float* rstd, float* dgamma, float* dbeta, void* workspace,
                          long workspace_bytes, int N, long V, int C, int lddy, int G, int mode, int relu,
                          int accumulate_params, hipStream_t stream) {
  GnGeom g;
  int r = gn_geom(g, N, V, C, G, mode);
  if (r != BTS_OK) return r;
  if (lddy < C) return BTS_ERR_ALIGN;
  if (workspace == nullptr) return BTS_ERR_WORKSPACE;
  if (g.generic || lddy % 4 != 0) {
    if (workspace_bytes < (long)N * G * 2 * 4 + 64) return BTS_ERR_WORKSPACE;
    float* gc1 = reinterpret_cast<float*>(workspace);
    float* gc2 = gc1 + (long)N * G;
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_group_generic_kernel, dim3(N * G), dim3(256), 0, stream, x, dy, gamma, beta, mean, rstd, gc1, gc2,
                       g.E, g.L, C, G, g.cg, lddy, mode, relu);
    BTS_LAUNCH_CHECK();
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_param_generic_kernel, dim3(C), dim3(256), 0, stream, x, dy, gamma, beta, mean, rstd, dgamma, dbeta,
                       N, g.E, g.L, C, G, g.cg, lddy, mode, relu, accumulate_params);
    BTS_LAUNCH_CHECK();
    const long total = (long)N * g.E;
    int gb = (int)((total + 255) / 256);
    if (gb > 8192) gb = 8192;
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_apply_generic_kernel, dim3(gb), dim3(256), 0, stream, x, dy, dx, gamma, beta, mean, rstd, gc1, gc2,
                       total, g.E, g.L, C, G, g.cg, lddy, mode, relu);
    BTS_LAUNCH_CHECK();
    return BTS_OK;
  }
  if ((((uintptr_t)x) & 15) || (((uintptr_t)dy) & 15) || (((uintptr_t)dx) & 15)) return BTS_ERR_ALIGN;
  const long part_bytes = bts_gn_workspace(N, V, C, G, mode);
  const long extra = (long)N * C * 2 * 8 + (long)N * G * 2 * 4 + 64;
  if (workspace_bytes < part_bytes + extra) return BTS_ERR_WORKSPACE;
  double* partial = reinterpret_cast<double*>(workspace);
  double* scratch = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + ((part_bytes + 15) & ~15L));
  float* c1 = reinterpret_cast<float*>(scratch + (long)N * C * 2);
  float* c2 = c1 + (long)N * G;
  const bool slab = (mode == BTS_GN_SLAB);
  (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_reduce_kernel, dim3(g.B, slab ? N * G : N), dim3(256), 0, stream, x, dy, gamma, beta, mean,
                     rstd, partial, g.E, g.L, g.span, C, G, g.cg, lddy, mode, relu);
  BTS_LAUNCH_CHECK();
  if (slab && g.cg <= 256 && 256 % g.cg == 0) {
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_finalize_slab_kernel, dim3(G), dim3(256), 0, stream, partial, gamma, dgamma, dbeta, c1, c2, N, G, g.B,
                       g.cg, (double)g.L, accumulate_params);
    BTS_LAUNCH_CHECK();
  } else {
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_finalize_a_kernel, dim3((N * C + 3) / 4), dim3(256), 0, stream, partial, scratch, N, g.B, C, G, mode);
    BTS_LAUNCH_CHECK();
    (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(1), dim3(256), 0, stream, gamma, dgamma, dbeta, c1, c2, scratch, N, C, G,
                       (double)g.L, accumulate_params);
    BTS_LAUNCH_CHECK();
  }
  if (slab && g.L % 1024 == 0 && 1024 % C == 0) {
    const long cpu = g.L / 1024;
    const int cpb = gn_stream_cpb(cpu);
    const long nblk = (long)N * G * cpu / cpb;
    if (nblk <= 0x7fffffffL) {
      (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_apply_slab_stream_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, x, dy, dx, gamma, beta,
                         mean, rstd, c1, c2, cpu, cpb, C, g.cg, G, relu, lddy);
      BTS_LAUNCH_CHECK();
      return BTS_OK;
    }
  }
  const long total4 = (long)N * g.E / 4;
  int blocks = (int)((total4 + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  (void)hipGetLastError(); hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(blocks), dim3(256), 0, stream, x, dy, dx, gamma, beta, mean, rstd, c1, c2,
                     total4, g.E, g.L, C, G, g.cg, lddy, mode, relu);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" long bts_gn_bwd_workspace(int N, long V, int C, int G, int mode) {
  const long p = bts_gn_workspace(N, V, C, G, mode);
  if (p < 0) return -1;
  return ((p + 15) & ~15L) + (long)N * C * 2 * 8 + (long)N * G * 2 * 4 + 64;
}
