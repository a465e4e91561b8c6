// Rigid co-registration of a scan's modalities by mutual information: the two device passes of bts_amd.coreg.
//
//   bts_quantize_bins   q = clamp(floor((double(v) - lo) * bins / (hi - lo)), 0, bins - 1), one byte per voxel, fp64, each operation rounded
//                       once (a NaN gives bin 0).
//   bts_joint_hist_pv   K joint histograms of a binned fixed and a binned moving volume, one per candidate 3 x 4 map, by partial-volume
//                       interpolation: nothing is interpolated, the eight neighbours of a mapped point share its mass by integer weights.
//
// With Q = CR_Q = 32, for lattice point l of the fixed grid, f = o + l * s, a = qf[f]:
//   c_j = ((m[j][0] f0 + m[j][1] f1) + m[j][2] f2) + m[j][3]                        fp64, separate operations (no contraction)
//   the point counts only if 0 <= c_j <= N_j - 1 on all three axes (a NaN fails)
//   i_j = floor(c_j),  r_j = (int)floor((c_j - i_j) Q + 0.5)  in [0, Q]
//   corner (d0,d1,d2) in {0,1}^3: b = qm[min(i_j + d_j, N_j - 1)],  hist[k][a][b] += prod_j (d_j ? r_j : Q - r_j)
// so every counted point adds exactly Q^3 = 32768 and the overlap is sum(hist[k]) / Q^3.  All sums are integers: the same bits in every
// run, whatever the order.
//
// Layout: the grid is (runs of CR_PTS lattice points) x (candidates); a thread owns CR_PTS / 256 points, consecutive threads consecutive
// points along the lattice's last axis.  A workgroup counts into 32-bit LDS histograms, one private copy per wave where bins^2 allows
// (four at bins <= 32), then adds the non-zero bins to the 64-bit global histogram with integer atomics (casenorm.hip's pattern).
// Most of a skull-stripped scan's mass is background on background, one LDS address: bin (0,0) is counted in a register per thread, and
// a point whose eight neighbours share one bin (any homogeneous region) makes one LDS add of Q^3 in place of eight.
// A 32-bit counter holds 2^32 / Q^3 = 131072 points; a workgroup counts at most CR_PTS of them for one candidate (static_assert below).
// The moving volume is gathered byte-wise straight from global memory: neighbouring lattice points share cache lines, and a scan fits in L2.
#include <math.h>
#include "common.h"
#include "bts_internal.h"

#pragma clang fp contract(off)   // the contract is separate fp64 operations, each rounded once

#define CR_Q 32
#define CR_PTS 2048          // lattice points per workgroup and candidate
#define CR_MAXK 32
#define CR_MAXBINS 64
#define CR_LDS_WORDS (CR_MAXBINS * CR_MAXBINS)   // 16 KB: one histogram at 64 bins, one per wave at <= 32
static_assert((long)CR_PTS * CR_Q * CR_Q * CR_Q < (1L << 32), "a workgroup's 32-bit LDS counters must hold all of its points in one bin");
static_assert(CR_PTS % 256 == 0, "whole rounds of the workgroup");

__global__ __launch_bounds__(256) void cr_quantize_kernel(const float* __restrict__ x, unsigned char* __restrict__ q, long n, double lo,
                                                          double range, double bins) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    const double t = floor(((double)x[i] - lo) * bins / range);
    q[i] = (unsigned char)(t >= 0.0 ? (t < bins - 1.0 ? t : bins - 1.0) : 0.0);   // a NaN fails t >= 0
  }
}

__global__ __launch_bounds__(256) void cr_zero_kernel(unsigned long long* __restrict__ h, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) h[i] = 0ull;
}

struct CrParams {
  const unsigned char* qf;
  const unsigned char* qm;
  unsigned long long* hist;
  long npts;                // n0 * n1 * n2
  int Hf, Wf;               // fixed extents below the first axis
  int Nm[3];                // moving extents
  int o[3], s[3], n1, n2;   // the lattice
  int bins, copies;         // LDS histograms per workgroup: wave w counts into copy w % copies
  double m[CR_MAXK * 12];
};

__global__ __launch_bounds__(256) void cr_joint_hist_kernel(const CrParams p) {
  __shared__ unsigned lh[CR_LDS_WORDS];
  const int bins = p.bins, nb2 = bins * bins, used = nb2 * p.copies;
  for (int i = threadIdx.x; i < used; i += 256) lh[i] = 0u;
  __syncthreads();
  const double* m = p.m + blockIdx.y * 12;
  unsigned* mine = lh + ((threadIdx.x >> 6) % p.copies) * nb2;
  const double hi0 = (double)(p.Nm[0] - 1), hi1 = (double)(p.Nm[1] - 1), hi2 = (double)(p.Nm[2] - 1);
  const long HWm = (long)p.Nm[1] * p.Nm[2];
  const long base = (long)blockIdx.x * CR_PTS;
  unsigned zero = 0u;        // bin (0,0) of this thread: at most CR_PTS / 256 points of Q^3 each
  for (int r = 0; r < CR_PTS / 256; ++r) {
    const long l = base + r * 256 + threadIdx.x;
    if (l >= p.npts) break;
    const int l2 = (int)(l % p.n2);
    const long row = l / p.n2;
    const int l1 = (int)(row % p.n1), l0 = (int)(row / p.n1);
    const int f0 = p.o[0] + l0 * p.s[0], f1 = p.o[1] + l1 * p.s[1], f2 = p.o[2] + l2 * p.s[2];
    const double c0 = ((m[0] * (double)f0 + m[1] * (double)f1) + m[2] * (double)f2) + m[3];
    const double c1 = ((m[4] * (double)f0 + m[5] * (double)f1) + m[6] * (double)f2) + m[7];
    const double c2 = ((m[8] * (double)f0 + m[9] * (double)f1) + m[10] * (double)f2) + m[11];
    if (!(c0 >= 0.0 && c0 <= hi0 && c1 >= 0.0 && c1 <= hi1 && c2 >= 0.0 && c2 <= hi2)) continue;
    const unsigned top = (unsigned)bins - 1u;
    const unsigned a = min((unsigned)p.qf[((long)f0 * p.Hf + f1) * p.Wf + f2], top);   // a byte past the bins stays inside the histogram
    const double e0 = floor(c0), e1 = floor(c1), e2 = floor(c2);
    const int i0 = (int)e0, i1 = (int)e1, i2 = (int)e2;      // in [0, N - 1]
    const int r0 = (int)floor((c0 - e0) * (double)CR_Q + 0.5), r1 = (int)floor((c1 - e1) * (double)CR_Q + 0.5),
              r2 = (int)floor((c2 - e2) * (double)CR_Q + 0.5);
    const int j0 = i0 + 1 < p.Nm[0] ? i0 + 1 : i0, j1 = i1 + 1 < p.Nm[1] ? i1 + 1 : i1, j2 = i2 + 1 < p.Nm[2] ? i2 + 1 : i2;
    const unsigned char* pa = p.qm + (long)i0 * HWm;
    const unsigned char* pb = p.qm + (long)j0 * HWm;
    const long ra = (long)i1 * p.Nm[2], rb = (long)j1 * p.Nm[2];
    unsigned b[8];
    b[0] = pa[ra + i2]; b[1] = pa[ra + j2]; b[2] = pa[rb + i2]; b[3] = pa[rb + j2];
    b[4] = pb[ra + i2]; b[5] = pb[ra + j2]; b[6] = pb[rb + i2]; b[7] = pb[rb + j2];
    bool same = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = min(b[k], top);
#pragma unroll
    for (int k = 1; k < 8; ++k) same &= b[k] == b[0];
    unsigned* rowa = mine + a * bins;
    if (same) {                                               // the eight weights add up to Q^3
      if ((a | b[0]) == 0u) zero += CR_Q * CR_Q * CR_Q;
      else atomicAdd(rowa + b[0], (unsigned)(CR_Q * CR_Q * CR_Q));
      continue;
    }
    const unsigned w0[2] = {(unsigned)(CR_Q - r0), (unsigned)r0}, w1[2] = {(unsigned)(CR_Q - r1), (unsigned)r1},
                   w2[2] = {(unsigned)(CR_Q - r2), (unsigned)r2};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned w = w0[k >> 2] * w1[(k >> 1) & 1] * w2[k & 1];
      if (w == 0u) continue;
      if ((a | b[k]) == 0u) zero += w;
      else atomicAdd(rowa + b[k], w);
    }
  }
  if (zero) atomicAdd(mine, zero);
  __syncthreads();
  unsigned long long* out = p.hist + (long)blockIdx.y * nb2;
  for (int i = threadIdx.x; i < nb2; i += 256) {
    unsigned v = 0u;                                          // <= CR_PTS * Q^3 over all copies: no overflow
    for (int c = 0; c < p.copies; ++c) v += lh[c * nb2 + i];
    if (v) atomicAdd(out + i, (unsigned long long)v);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
extern "C" int bts_quantize_bins(const float* x, uint8_t* q, long n, double lo, double hi, int bins, hipStream_t stream) {
  if (n <= 0 || bins < 2 || bins > CR_MAXBINS) return BTS_ERR_SHAPE;
  if (!(hi > lo) || !isfinite(lo) || !isfinite(hi) || !isfinite(hi - lo)) return BTS_ERR_SHAPE;   // a NaN fails hi > lo
  if (x == nullptr || q == nullptr) return BTS_ERR_SHAPE;
  long blocks = (n + 255) / 256;
  if (blocks > 262144) blocks = 262144;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cr_quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, q, n, lo, hi - lo, (double)bins);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_joint_hist_pv(const uint8_t* qf, int Df, int Hf, int Wf, const uint8_t* qm, int Dm, int Hm, int Wm, int o0, int o1,
                                 int o2, int s0, int s1, int s2, int n0, int n1, int n2, const double* m12, int K, int bins,
                                 unsigned long long* hist, hipStream_t stream) {
  if (Df < 1 || Hf < 1 || Wf < 1 || Dm < 1 || Hm < 1 || Wm < 1) return BTS_ERR_SHAPE;
  if ((long)Df * Hf * Wf > 0x7fffffffL || (long)Dm * Hm * Wm > 0x7fffffffL) return BTS_ERR_SHAPE;
  const int F[3] = {Df, Hf, Wf}, o[3] = {o0, o1, o2}, s[3] = {s0, s1, s2}, n[3] = {n0, n1, n2};
  for (int a = 0; a < 3; ++a) {
    if (o[a] < 0 || s[a] < 1 || n[a] < 1 || o[a] >= F[a]) return BTS_ERR_SHAPE;
    if ((long)o[a] + (long)(n[a] - 1) * s[a] > (long)F[a] - 1) return BTS_ERR_SHAPE;   // the last lattice point lies inside the fixed volume
  }
  if (K < 1 || K > CR_MAXK || bins < 2 || bins > CR_MAXBINS) return BTS_ERR_SHAPE;
  if (qf == nullptr || qm == nullptr || m12 == nullptr || hist == nullptr) return BTS_ERR_SHAPE;
  CrParams p;
  p.qf = qf; p.qm = qm; p.hist = hist;
  p.npts = (long)n0 * n1 * n2;                                // <= Df * Hf * Wf < 2^31
  p.Hf = Hf; p.Wf = Wf;
  p.Nm[0] = Dm; p.Nm[1] = Hm; p.Nm[2] = Wm;
  for (int a = 0; a < 3; ++a) { p.o[a] = o[a]; p.s[a] = s[a]; }
  p.n1 = n1; p.n2 = n2;
  p.bins = bins;
  const int fit = CR_LDS_WORDS / (bins * bins);
  p.copies = fit < 4 ? fit : 4;
  for (int k = 0; k < K * 12; ++k) p.m[k] = m12[k];
  for (int k = K * 12; k < CR_MAXK * 12; ++k) p.m[k] = 0.0;
  const int total = K * bins * bins;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cr_zero_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, hist, total);
  BTS_LAUNCH_CHECK();
  const long runs = (p.npts + CR_PTS - 1) / CR_PTS;
  hipLaunchKernelGGL(cr_joint_hist_kernel, dim3((unsigned)runs, (unsigned)K), dim3(256), 0, stream, p);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
