// Bodies of finalize kernels that exist on their own (groupnorm.hip, se.hip; lowp_norm.hip, lowp_point.hip) and as the roles of ONE launch
// in the fused block backward (block_bwd.hip, lowp_block.hip: they only need the reduce pass's partials, and each costs a ~5 us launch on
// the main stream's chain) -- and the per-block bias-gradient sum the 16-bit backward apply kernels of lowp_norm.hip and lowp_block.hip share.
#pragma once
#include "common.h"

// slab-mode GroupNorm backward finalize for group g: class sums over the blocks -> c1, c2 per sample; over the samples -> dgamma, dbeta.
// One 256-thread workgroup; sh: 512 doubles of LDS.  cg = C / G is a power of two <= 256.
__device__ __forceinline__ void gn_bwd_finalize_slab_body(const double* partial, const float* gamma, float* dgamma, float* dbeta, float* c1,
                                                          float* c2, int N, int G, int B, int cg, double L, int accum, int g, double* sh) {
  const int j = threadIdx.x % cg, sl = threadIdx.x / cg, S = 256 / cg;
  double ga = 0.0, gb = 0.0;
  for (int n = 0; n < N; ++n) {
    const long unit = (long)n * G + g;
    double sa = 0.0, sb = 0.0;
    for (int b = sl; b < B; b += S) {
      const double* o = partial + ((unit * B + b) * cg + j) * 2;
      sa += o[0]; sb += o[1];
    }
    __syncthreads();
    sh[threadIdx.x * 2] = sa; sh[threadIdx.x * 2 + 1] = sb;
    __syncthreads();
    if (sl == 0) {
      sa = 0.0; sb = 0.0;
      for (int s2 = 0; s2 < S; ++s2) { sa += sh[(s2 * cg + j) * 2]; sb += sh[(s2 * cg + j) * 2 + 1]; }
      ga += sa; gb += sb;
    }
    __syncthreads();
    if (sl == 0) {
      sh[j * 2] = (double)gamma[g * cg + j] * sb;       // -> c1
      sh[j * 2 + 1] = (double)gamma[g * cg + j] * sa;   // -> c2
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double s1 = 0.0, s2 = 0.0;
      for (int q = 0; q < cg; ++q) { s1 += sh[q * 2]; s2 += sh[q * 2 + 1]; }
      c1[unit] = (float)(s1 / L);
      c2[unit] = (float)(s2 / L);
    }
  }
  if (sl == 0) {
    const int idx = g * cg + j;
    if (dgamma) dgamma[idx] = accum ? dgamma[idx] + (float)ga : (float)ga;
    if (dbeta) dbeta[idx] = accum ? dbeta[idx] + (float)gb : (float)gb;
  }
}

// gate backward stage 2a for the four (n, c) pairs of workgroup `blk`: one wave per pair sums the per-block partials
__device__ __forceinline__ void se_bwd_partial_reduce_body(const double* partial, double* red, int N, int B, int F, int blk) {
  const int lane = threadIdx.x & 63;
  const int i = blk * 4 + (threadIdx.x >> 6);
  if (i >= N * F) return;
  const int n = i / F, c = i % F;
  double a = 0.0, b = 0.0;
  const double2* pp = reinterpret_cast<const double2*>(partial) + (long)n * B * F + c;      // pair (n, k, c) at pp[k * F]
  int k = lane;
  for (; k + 7 * 64 < B; k += 8 * 64) {      // eight loads in flight, added in index order (the fused block backward leaves 2048 rows per sample)
    double2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = pp[(long)(k + u * 64) * F];
#pragma unroll
    for (int u = 0; u < 8; ++u) { a += v[u].x; b += v[u].y; }
  }
  for (; k < B; k += 64) {
    const double2 v = pp[(long)k * F];
    a += v.x;
    b += v.y;
  }
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  if (lane == 0) { red[i * 2] = a; red[i * 2 + 1] = b; }
}

// gate backward, the sums over the samples (dW2, dW1, dw_sp) for workgroup `blk` of ceil(R * F / 256): se.hip's se_mlp_bwd_param_kernel, and one
// role of the 16-bit block backward's tail launch (lowp_block.hip).  red: [N][F][2] summed partials; scratch: dz2 [N][F] | dz1 [N][R] of the per-sample pass.
__device__ __forceinline__ void se_mlp_bwd_param_body(const double* red, const float* gap, const float* hbuf, float* dw1, float* dw2, float* dwsp,
                                                      const double* scratch, int N, int F, int R, int accum, int blk) {
  const double* dz2 = scratch;
  const double* dz1 = scratch + (long)N * F;
  const int i = blk * 256 + threadIdx.x;
  if (i < R * F) {
    {
      const int k = i / F, c = i % F;
      double s = 0.0;
      for (int n = 0; n < N; ++n) s += (double)hbuf[n * R + k] * dz2[n * F + c];
      dw2[i] = accum ? dw2[i] + (float)s : (float)s;
    }
    {
      const int c = i / R, k = i % R;
      double s = 0.0;
      for (int n = 0; n < N; ++n) s += (double)gap[n * F + c] * dz1[n * R + k];
      dw1[i] = accum ? dw1[i] + (float)s : (float)s;
    }
  }
  if (i < F) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += red[((long)n * F + i) * 2 + 1];
    dwsp[i] = accum ? dwsp[i] + (float)s : (float)s;
  }
}

// ---- the 16-bit engine ----
// Bias gradient of the conv that produced the tensor a backward apply pass writes (its dy): db[c] = sum over voxels and samples.  The
// apply kernels walk octets with a stride that is a multiple of the channel count, so a thread's channel octet never changes: it keeps
// eight running sums, the block adds the threads of equal octet in LDS (fixed order) and leaves one fp64 partial row per block;
// lp_dbias_finalize_kernel adds the rows in block order.  (Round 2 read every such dy a second time: bts_lp_colsum, 4.5 ms per step.)
__device__ __forceinline__ void lp_dbias_block(const float (&cs)[8], int oct, int noct, double* part_row, float* sh /* [256][8] */) {
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) sh[threadIdx.x * 8 + e] = cs[e];
  __syncthreads();
  if ((int)threadIdx.x < noct * 8) {
    const int o = threadIdx.x >> 3, e = threadIdx.x & 7;
    double s = 0.0;
    for (int t = o; t < 256; t += noct) s += (double)sh[t * 8 + e];     // threads t = o (mod noct) hold octet o
    part_row[o * 8 + e] = s;
  }
  (void)oct;
}
// one workgroup per channel c: threads split the block rows, fixed-order combine (sh: 4 doubles of LDS)
__device__ __forceinline__ void lp_dbias_finalize_body(const double* part, float* db, int nblocks, int C, int accum, int c, double* sh) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += part[(long)b * C + c];
  s = block_sum_f64(s, sh);
  if (threadIdx.x == 0) db[c] = accum ? db[c] + (float)s : (float)s;
}

// one block per group g: for every sample the class sums over the blocks -> c1, c2; the sums over the samples -> dgamma, dbeta.
// Up to 256 / cg samples side by side (thread = (slice of the blocks, sample, class)): the loop over the samples of a batch of 8 was
// eight dependent rounds, 15 us on the critical path between the reduce and the apply pass of every GroupNorm backward.
__device__ __forceinline__ void lp_gn_bwd_finalize_body(const double* partial, const float* gamma, float* dgamma, float* dbeta, float* c1,
                                                        float* c2, int N, int G, int B, int cg, double L, int accum, int g, double* sh,
                                                        double* tot /* [sample slot][class] totals of the current round */) {
  const int t = threadIdx.x;
  int Np = 1;
  while (Np * 2 <= N && cg * Np * 2 <= 256) Np *= 2;
  const int S = 256 / (cg * Np);
  const int j = t % cg, nl = (t / cg) % Np, sl = t / (cg * Np);
  double ga = 0.0, gb = 0.0;     // running dgamma / dbeta of class t (threads t < cg)
  for (int n0 = 0; n0 < N; n0 += Np) {
    const int n = n0 + nl;
    double sa = 0.0, sb = 0.0;
    if (n < N) {
      const long unit = (long)n * G + g;
      for (int b = sl; b < B; b += S) {
        const double* o = partial + ((unit * B + b) * cg + j) * 2;
        sa += o[0]; sb += o[1];
      }
    }
    __syncthreads();
    sh[t * 2] = sa; sh[t * 2 + 1] = sb;
    __syncthreads();
    if (sl == 0) {      // slices in fixed order
      sa = 0.0; sb = 0.0;
      for (int s2 = 0; s2 < S; ++s2) { sa += sh[((s2 * Np + nl) * cg + j) * 2]; sb += sh[((s2 * Np + nl) * cg + j) * 2 + 1]; }
      tot[(nl * cg + j) * 2] = sa; tot[(nl * cg + j) * 2 + 1] = sb;
    }
    __syncthreads();
    if (t < Np && n0 + t < N) {      // c1, c2 of sample n0 + t
      double s1 = 0.0, s2 = 0.0;
      for (int q = 0; q < cg; ++q) {
        s1 += (double)gamma[g * cg + q] * tot[(t * cg + q) * 2 + 1];
        s2 += (double)gamma[g * cg + q] * tot[(t * cg + q) * 2];
      }
      const long unit = (long)(n0 + t) * G + g;
      c1[unit] = (float)(s1 / L);
      c2[unit] = (float)(s2 / L);
    }
    if (t < cg) {                    // samples in fixed order
      for (int q = 0; q < Np && n0 + q < N; ++q) { ga += tot[(q * cg + t) * 2]; gb += tot[(q * cg + t) * 2 + 1]; }
    }
  }
  if (t < cg) {
    const int idx = g * cg + t;
    dgamma[idx] = accum ? dgamma[idx] + (float)ga : (float)ga;
    dbeta[idx] = accum ? dbeta[idx] + (float)gb : (float)gb;
  }
}
