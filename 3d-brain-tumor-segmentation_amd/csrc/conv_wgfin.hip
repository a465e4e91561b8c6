// The finalize pass of the fp32 weight gradient: dW[t][pc][qc] (+)= the sum of the per-workgroup partial tiles the weight-gradient kernels
// (conv_wgrad.hip, conv_wgw.hip, conv_k1w.hip) left in the workspace, [nsp][npct][nqct][ntiles][32][32], and db (+)= the sum of their
// bias partials [nsp][nqct][32] -- fp64 accumulate in a fixed order (bitwise reproducible; no float atomics), stored in the reference
// layout of the call's form.  Two kernels share the two rules below and differ in how they walk the partials.
#include "wgrad_plan.h"

// Where row (t, pc) of channel tile qct lies inside one workgroup's partials (floats; its 32 qc are consecutive): a tile per tap, or --
// cpad < 32 -- packed (tap, channel) rows
__device__ __forceinline__ long wfin_partial_off(const WfinParams& f, int t, int pc, int qct) {
  if (f.cpad == 32) return ((((long)(pc >> 5)) * f.nqct + qct) * f.ntiles + t) * 1024 + (pc & 31) * 32;
  const int ci = t * f.cpad + pc;
  return ((long)qct * f.ntiles + (ci >> 5)) * 1024 + (ci & 31) * 32;
}
// Where the sum goes.  Folded slab channel c (on the P or the Q axis: fold_axis) maps to reference channel c+shift and, if
// c >= dup_start, also to c-dup_start (both copies of the duplicated slice see the same input: encoder.py:83-87).
__device__ __forceinline__ void wfin_store(const WfinParams& f, int t, int pc, int qc, float tot) {
  const int pr = (f.fold_axis == 1) ? pc + f.shift : pc;
  const int qr = (f.fold_axis == 2) ? qc + f.shift : qc;
  float* d1 = f.dw + t * f.sT + pr * f.sP + qr * f.sQ;
  *d1 = f.accum ? (*d1 + tot) : tot;
  if (f.shift > 0) {
    if (f.fold_axis == 1 && pc >= f.dup_start) {
      float* d2 = f.dw + t * f.sT + (pc - f.dup_start) * f.sP + qr * f.sQ;
      *d2 = f.accum ? (*d2 + tot) : tot;
    } else if (f.fold_axis == 2 && qc >= f.dup_start) {
      float* d2 = f.dw + t * f.sT + pr * f.sP + (qc - f.dup_start) * f.sQ;
      *d2 = f.accum ? (*d2 + tot) : tot;
    }
  }
}

// One block per row (32 consecutive qc of one (t, pc, qct)): 256 threads = 8 float4 columns x 32 partial-lanes, every lane streams its
// share of the nsp partials (4 independent 16-byte loads in flight), fp64 accumulate, fixed-order combine through LDS.  The pass is
// pure HBM streaming.
__global__ __launch_bounds__(256) void wgrad_finalize_kernel(const WfinParams f) {
  __shared__ double sh[32][33];
  const int q4 = threadIdx.x & 7, wl = threadIdx.x >> 3;
  const long rows = (long)f.ntaps * f.Cp * f.nqct;
  const long wgStride = (long)f.npct * f.nqct * f.ntiles * 1024;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int qct = (int)(row % f.nqct);
    long r = row / f.nqct;
    const int pc = (int)(r % f.Cp);
    const int t = (int)(r / f.Cp);
    const float* src = f.partial + wfin_partial_off(f, t, pc, qct) + q4 * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // fp64 combine of the per-workgroup fp32 partials
    int w = wl;
    for (; w + 96 < f.nsp; w += 128) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + (long)w * wgStride);
      const f32x4 b = *reinterpret_cast<const f32x4*>(src + (long)(w + 32) * wgStride);
      const f32x4 c = *reinterpret_cast<const f32x4*>(src + (long)(w + 64) * wgStride);
      const f32x4 d = *reinterpret_cast<const f32x4*>(src + (long)(w + 96) * wgStride);
      s0 += (double)a[0]; s1 += (double)a[1]; s2 += (double)a[2]; s3 += (double)a[3];
      s0 += (double)b[0]; s1 += (double)b[1]; s2 += (double)b[2]; s3 += (double)b[3];
      s0 += (double)c[0]; s1 += (double)c[1]; s2 += (double)c[2]; s3 += (double)c[3];
      s0 += (double)d[0]; s1 += (double)d[1]; s2 += (double)d[2]; s3 += (double)d[3];
    }
    for (; w < f.nsp; w += 32) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + (long)w * wgStride);
      s0 += (double)a[0]; s1 += (double)a[1]; s2 += (double)a[2]; s3 += (double)a[3];
    }
    __syncthreads();
    sh[wl][q4 * 4 + 0] = s0; sh[wl][q4 * 4 + 1] = s1; sh[wl][q4 * 4 + 2] = s2; sh[wl][q4 * 4 + 3] = s3;
    __syncthreads();
    if (threadIdx.x < 32) {
      const int e = threadIdx.x;
      double totd = sh[0][e];
#pragma unroll
      for (int k = 1; k < 32; ++k) totd += sh[k][e];
      const int qc = qct * 32 + e;
      if (qc < f.Cq) wfin_store(f, t, pc, qc, (float)totd);
    }
  }
  // bias: block qct combines the per-workgroup fp64 column sums of its 32 channels (32 channels x 8 partial-lanes)
  if (f.db && (int)blockIdx.x < f.nqct) {
    const int e = threadIdx.x & 31, l8 = threadIdx.x >> 5, qct = blockIdx.x;
    double s = 0.0;
    for (int w = l8; w < f.nsp; w += 8) s += f.partial_b[((long)w * f.nqct + qct) * 32 + e];
    __syncthreads();
    sh[l8][e] = s;
    __syncthreads();
    if (l8 == 0 && qct * 32 + e < f.Cq) {
      double tot = sh[0][e];
#pragma unroll
      for (int k = 1; k < 8; ++k) tot += sh[k][e];
      const int i = qct * 32 + e;
      f.db[i] = f.accum ? (f.db[i] + (float)tot) : (float)tot;
    }
  }
}

// Same combine for few partials (nsp <= 16): one thread per output element, partials read coalesced along qc.
__global__ __launch_bounds__(256) void wgrad_finalize_flat_kernel(const WfinParams f) {
  const int nq = f.nqct * 32;
  const long total = (long)f.ntaps * f.Cp * nq;
  const long wgStride = (long)f.npct * f.nqct * f.ntiles * 1024;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int qc = (int)(i % nq);
    long r = i / nq;
    const int pc = (int)(r % f.Cp);
    const int t = (int)(r / f.Cp);
    if (qc >= f.Cq) continue;
    const long off = wfin_partial_off(f, t, pc, qc >> 5) + (qc & 31);
    double totd = 0.0;
    for (int w = 0; w < f.nsp; ++w) totd += (double)f.partial[w * wgStride + off];
    wfin_store(f, t, pc, qc, (float)totd);
  }
  if (f.db && blockIdx.x == 0) {
    for (int i = threadIdx.x; i < f.Cq; i += blockDim.x) {
      double s = 0.0;
      for (int w = 0; w < f.nsp; ++w) s += f.partial_b[((long)w * f.nqct + (i >> 5)) * 32 + (i & 31)];
      f.db[i] = f.accum ? (f.db[i] + (float)s) : (float)s;
    }
  }
}

// dw is in the reference layout with Cin_ref = Cin + dup_shift input channels.  Not profiled.
int bts_wgrad_finalize_(const WgCall& c, const WgChoice& ch, const WgradParams& p, float* dw, float* db, hipStream_t stream) {
  const WgradRoles& ro = ch.ro;
  WfinParams f;
  f.partial = p.partial; f.partial_b = p.partial_b; f.dw = dw; f.db = p.want_bias ? db : nullptr;
  f.nsp = ch.nsp; f.npct = ch.npct; f.nqct = ch.nqct; f.ntaps = ro.ntaps; f.ntiles = p.ntiles; f.cpad = p.cpad;
  f.Cp = ro.Cp; f.Cq = ro.Cq;
  // the layout by form: strides of the tap, the P and the Q channel in dw, and the axis the slab's fold lies on
  const int Cin_ref = c.Cin + c.dup_shift;
  f.sT = (long)Cin_ref * c.Cout;
  if (ro.transposed) { f.sP = Cin_ref; f.sQ = 1; f.fold_axis = 0; }     // (t, Cout, Cin): P = cout, Q = cin
  else if (ro.swapped) { f.sP = 1; f.sQ = c.Cout; f.fold_axis = 2; }     // (t, Cin, Cout): P = cout, Q = cin
  else { f.sP = c.Cout; f.sQ = 1; f.fold_axis = 1; }                     // (t, Cin, Cout): P = cin, Q = cout
  f.shift = c.dup_shift;
  f.dup_start = c.dup_shift > 0 ? c.dup_start : (1 << 30);
  f.accum = c.accumulate;
  const long rows = (long)ro.ntaps * ro.Cp * ch.nqct;
  (void)hipGetLastError();
  if (ch.nsp <= 16) {      // few partials: the flat kernel
    long blocks = (rows * 32 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(wgrad_finalize_flat_kernel, dim3((int)blocks), dim3(256), 0, stream, f);
  } else {
    const int blocks = (int)(rows < 4096 ? rows : 4096);
    hipLaunchKernelGGL(wgrad_finalize_kernel, dim3(blocks), dim3(256), 0, stream, f);
  }
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
