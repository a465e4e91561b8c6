// N4 bias-field correction of one MRI volume: the six device passes of bts_amd.n4 (Tustison et al. 2010).
//
// The field is exp of a cubic B-spline: along an axis of extent N with M mesh elements a voxel (or lattice point) of full-resolution
// index p has u = (p + 0.5) / N * M, cell i = min(floor(u), M - 1), t = u - i, and the weights
//   B0 = (1-t)^3 / 6,  B1 = (3 t^3 - 6 t^2 + 4) / 6,  B2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6,  B3 = t^3 / 6
// of the control points i .. i+3 out of M + 3 (n4_basis below is the one statement of it).  The working lattice is the strided sub-grid
// p = s / 2 + l s of the volume, n = (N - 1 - s / 2) / s + 1 points per axis.
//
//   bts_n4_log_lattice  v = log(double(x)) and a byte mask at the lattice points (inside: mask, x > 0, x finite)
//   bts_n4_range_hist   r = v - f, its exact min / max, and the histogram of r with linear two-bin weights as integers (2^24 per point)
//   bts_n4_residual     res = r - (E[i] (1 - o) + E[i+1] o), the sharpened table E looked up as the histogram was filled
//   bts_n4_fit          one level of multilevel B-spline approximation in GATHER form: a workgroup per control point sums
//                       w^3 z / S and w^2 over the lattice points of its 4-cell support only
//   bts_n4_eval         the spline at the lattice points, and per-workgroup sums of e = exp(f_new - f_old) and e^2 over the mask
//   bts_n4_apply        out = float(x / exp(spline)) at every voxel of the volume
//
// Arithmetic is fp64, every operation rounded on its own: contraction is switched off for the whole file by the pragma below, so the
// coordinate, the weights, r, the bin number and its fraction are the same bits as tests/n4_ref.py forms with numpy, and the histogram is
// equal to the reference's as integers.  No floating-point atomic anywhere: min / max go through integer atomics on the order-preserving
// 64-bit key of a double, the histogram is integer (64-bit counters in LDS, then in global memory, coreg.hip's pattern), and every
// floating sum has a fixed order (a thread's own points in index order, then block_sum_f64).  The same input gives the same bits in every run.
#include <math.h>
#include "common.h"
#include "bts_internal.h"

#pragma clang fp contract(off)   // separate fp64 operations, each rounded once: no fused multiply-add in this file

#define N4_Q 16777216.0          // 2^24: what one masked lattice point adds to the histogram
#define N4_MAXBINS 1024
#define N4_MAXN 512              // lattice points per axis whose weights the fit kernel keeps in LDS
#define N4_MAXMESH 64            // mesh elements per axis (six dyadic levels from mesh 2)
#define N4_PTS 1024              // lattice points per workgroup of the point-owning kernels, four per thread
#define N4_ROWS 32               // rows of the volume per workgroup of the apply kernel, at most
#define N4_XRUN 512              // voxels along x per workgroup of the apply kernel, at most
static_assert(N4_PTS % 256 == 0, "whole rounds of the workgroup");

struct N4Geo {
  int N[3], s[3], o[3], n[3], M[3];   // extent, lattice stride, origin and count, mesh elements
};

__device__ __forceinline__ int n4_basis(int p, int N, int M, double w[4]) {
  const double u = ((double)p + 0.5) / (double)N * (double)M;
  int i = (int)floor(u);
  if (i > M - 1) i = M - 1;
  const double t = u - (double)i;
  const double t2 = t * t, t3 = t2 * t, m = 1.0 - t;
  w[0] = ((m * m) * m) / 6.0;
  w[1] = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
  w[2] = (((3.0 * t2 - 3.0 * t3) + 3.0 * t) + 1.0) / 6.0;
  w[3] = t3 / 6.0;
  return i;
}

// the order-preserving 64-bit key of a double (no NaN among the values compared)
__device__ __forceinline__ unsigned long long n4_key(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double n4_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// ---- lattice gather ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void n4_log_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask, const N4Geo g,
                                                     double* __restrict__ v, unsigned char* __restrict__ lm, long npts) {
  const long l = blockIdx.x * 256L + threadIdx.x;
  if (l >= npts) return;
  const int l2 = (int)(l % g.n[2]);
  const long row = l / g.n[2];
  const int l1 = (int)(row % g.n[1]), l0 = (int)(row / g.n[1]);
  const long idx = ((long)(g.o[0] + l0 * g.s[0]) * g.N[1] + (g.o[1] + l1 * g.s[1])) * g.N[2] + (g.o[2] + l2 * g.s[2]);
  const float xv = x[idx];
  const bool ok = xv > 0.0f && xv <= 3.4028234663852886e38f && (mask == nullptr || mask[idx] != 0);   // a NaN fails xv > 0
  v[l] = ok ? log((double)xv) : 0.0;
  lm[l] = ok ? 1 : 0;
}

// ---- range and histogram -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void n4_init_kernel(unsigned long long* __restrict__ keys, long long* __restrict__ hist, int bins) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < bins) hist[i] = 0ll;
  if (i == 0) { keys[0] = ~0ull; keys[1] = 0ull; }
}

__global__ __launch_bounds__(256) void n4_range_kernel(const double* __restrict__ v, const double* __restrict__ f,
                                                       const unsigned char* __restrict__ lm, long npts, double* __restrict__ r,
                                                       unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long sk[2];
  if (threadIdx.x == 0) { sk[0] = ~0ull; sk[1] = 0ull; }
  __syncthreads();
  unsigned long long kmin = ~0ull, kmax = 0ull;
  const long base = (long)blockIdx.x * N4_PTS;
  for (int j = 0; j < N4_PTS / 256; ++j) {
    const long l = base + j * 256 + threadIdx.x;
    if (l >= npts) break;
    double d = 0.0;
    if (lm[l]) {
      d = v[l] - f[l];
      const unsigned long long k = n4_key(d);
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
    r[l] = d;
  }
  if (kmax != 0ull) { atomicMin(&sk[0], kmin); atomicMax(&sk[1], kmax); }
  __syncthreads();
  if (threadIdx.x == 0 && sk[1] != 0ull) { atomicMin(&keys[0], sk[0]); atomicMax(&keys[1], sk[1]); }
}

// c = (r - lo) / sl, i = min(floor(c), bins - 2), o = c - i; everything in bin 0 where hi == lo
__device__ __forceinline__ int n4_bin(double r, double lo, double sl, int bins, double* o) {
  if (!(sl > 0.0)) { *o = 0.0; return 0; }
  const double c = (r - lo) / sl;
  int i = (int)floor(c);
  if (i > bins - 2) i = bins - 2;
  if (i < 0) i = 0;
  *o = c - (double)i;
  return i;
}

__global__ __launch_bounds__(256) void n4_hist_kernel(const double* __restrict__ r, const unsigned char* __restrict__ lm, long npts,
                                                      int bins, const unsigned long long* __restrict__ keys, double* __restrict__ lohi,
                                                      long long* __restrict__ hist) {
  __shared__ unsigned long long lh[N4_MAXBINS];
  for (int i = threadIdx.x; i < bins; i += 256) lh[i] = 0ull;
  __syncthreads();
  const bool any = keys[1] != 0ull;
  const double lo = any ? n4_unkey(keys[0]) : (double)INFINITY, hi = any ? n4_unkey(keys[1]) : -(double)INFINITY;
  if (blockIdx.x == 0 && threadIdx.x == 0) { lohi[0] = lo; lohi[1] = hi; }
  const double sl = any ? (hi - lo) / (double)(bins - 1) : 0.0;
  const long base = (long)blockIdx.x * N4_PTS;
  for (int j = 0; j < N4_PTS / 256; ++j) {
    const long l = base + j * 256 + threadIdx.x;
    if (l >= npts) break;
    if (!lm[l]) continue;
    double o;
    const int i = n4_bin(r[l], lo, sl, bins, &o);
    long long q = (long long)rint(o * N4_Q);
    q = q < 0 ? 0 : (q > 16777216ll ? 16777216ll : q);
    if (q != 16777216ll) atomicAdd(&lh[i], (unsigned long long)(16777216ll - q));
    if (q != 0) atomicAdd(&lh[i + 1], (unsigned long long)q);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += 256)
    if (lh[i]) atomicAdd((unsigned long long*)hist + i, lh[i]);
}

// ---- residual ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void n4_residual_kernel(const double* __restrict__ r, const unsigned char* __restrict__ lm,
                                                          const double* __restrict__ E, long npts, int bins, double lo, double sl,
                                                          double* __restrict__ res) {
  const long l = blockIdx.x * 256L + threadIdx.x;
  if (l >= npts) return;
  double z = 0.0;
  if (lm[l]) {
    double o;
    const int i = n4_bin(r[l], lo, sl, bins, &o);
    z = r[l] - (E[i] * (1.0 - o) + E[i + 1] * o);
  }
  res[l] = z;
}

// ---- fit: one control point per workgroup ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void n4_fit_kernel(const double* __restrict__ res, const unsigned char* __restrict__ lm, const N4Geo g,
                                                     double* __restrict__ num, double* __restrict__ den, double* __restrict__ dphi,
                                                     double* __restrict__ phi) {
  __shared__ double wa[3][N4_MAXN];    // this control point's weight at lattice index l of axis a (0 outside its support)
  __shared__ double qa[3][N4_MAXN];    // the sum of the four squared weights of lattice index l of axis a
  __shared__ int lo[3], hi[3];         // the lattice indices [lo, hi) of the support per axis
  __shared__ double sh[4];
  const int P1 = g.M[1] + 3, P2 = g.M[2] + 3;
  const int cp[3] = {(int)(blockIdx.x / (P1 * P2)), (int)(blockIdx.x / P2 % P1), (int)(blockIdx.x % P2)};
  if (threadIdx.x < 3) { lo[threadIdx.x] = 0x7fffffff; hi[threadIdx.x] = 0; }
  __syncthreads();
  for (int a = 0; a < 3; ++a) {
    for (int l = threadIdx.x; l < g.n[a]; l += 256) {
      double w[4];
      const int i = n4_basis(g.o[a] + l * g.s[a], g.N[a], g.M[a], w);
      const int k = cp[a] - i;
      double mine = 0.0;
      if (k >= 0 && k <= 3) {
        mine = k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : w[3]));   // selects: a dynamic index would put w[] into scratch
        atomicMin(&lo[a], l);
        atomicMax(&hi[a], l + 1);
      }
      wa[a][l] = mine;
      qa[a][l] = ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) + w[3] * w[3];
    }
  }
  __syncthreads();
  double sn = 0.0, sd = 0.0;
  const int c0 = hi[0] - lo[0], c1 = hi[1] - lo[1], c2 = hi[2] - lo[2];
  if (c0 > 0 && c1 > 0 && c2 > 0) {
    // point e = threadIdx.x + 256 j of the box, last axis fastest, kept as three counters: a step of 256 is (d0, d1, d2) with carries,
    // so the loop divides nothing
    const int q = 256 / c2, d2 = 256 % c2, d1 = q % c1, d0 = q / c1;
    int a2 = (int)threadIdx.x % c2, a1 = ((int)threadIdx.x / c2) % c1, a0 = ((int)threadIdx.x / c2) / c1;
    while (a0 < c0) {
      const int l0 = lo[0] + a0, l1 = lo[1] + a1, l2 = lo[2] + a2;
      const long idx = ((long)l0 * g.n[1] + l1) * g.n[2] + l2;
      if (lm[idx]) {
        const double w = (wa[0][l0] * wa[1][l1]) * wa[2][l2];
        const double S = (qa[0][l0] * qa[1][l1]) * qa[2][l2];
        const double w2 = w * w;
        sn += ((w2 * w) * res[idx]) / S;
        sd += w2;
      }
      a2 += d2;
      int carry = a2 >= c2 ? 1 : 0;
      a2 -= carry * c2;
      a1 += d1 + carry;
      carry = a1 >= c1 ? 1 : 0;
      a1 -= carry * c1;
      a0 += d0 + carry;
    }
  }
  sn = block_sum_f64(sn, sh);
  sd = block_sum_f64(sd, sh);
  if (threadIdx.x == 0) {
    const double d = sd > 0.0 ? sn / sd : 0.0;
    num[blockIdx.x] = sn;
    den[blockIdx.x] = sd;
    dphi[blockIdx.x] = d;
    if (phi != nullptr) phi[blockIdx.x] = phi[blockIdx.x] + d;
  }
}

// ---- the spline at the lattice points ----------------------------------------------------------------------------------------------
__device__ __forceinline__ double n4_spline(const double* __restrict__ phi, int P1, int P2, int i0, int i1, int i2, const double w0[4],
                                            const double w1[4], const double w2[4]) {
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double ra = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double* p = phi + ((long)(i0 + a) * P1 + (i1 + b)) * P2 + i2;
      const double rb = ((w2[0] * p[0] + w2[1] * p[1]) + w2[2] * p[2]) + w2[3] * p[3];
      ra = ra + w1[b] * rb;
    }
    acc = acc + w0[a] * ra;
  }
  return acc;
}

__global__ __launch_bounds__(256) void n4_eval_kernel(const double* __restrict__ phi, const N4Geo g, const double* __restrict__ f_old,
                                                      const unsigned char* __restrict__ lm, long npts, double* __restrict__ f_new,
                                                      double* __restrict__ parts) {
  __shared__ double sh[4];
  double se = 0.0, se2 = 0.0;
  const long base = (long)blockIdx.x * N4_PTS;
  for (int j = 0; j < N4_PTS / 256; ++j) {
    const long l = base + j * 256 + threadIdx.x;
    if (l >= npts) break;
    const int l2 = (int)(l % g.n[2]);
    const long row = l / g.n[2];
    const int l1 = (int)(row % g.n[1]), l0 = (int)(row / g.n[1]);
    double w0[4], w1[4], w2[4];
    const int i0 = n4_basis(g.o[0] + l0 * g.s[0], g.N[0], g.M[0], w0);
    const int i1 = n4_basis(g.o[1] + l1 * g.s[1], g.N[1], g.M[1], w1);
    const int i2 = n4_basis(g.o[2] + l2 * g.s[2], g.N[2], g.M[2], w2);
    const double fn = n4_spline(phi, g.M[1] + 3, g.M[2] + 3, i0, i1, i2, w0, w1, w2);
    f_new[l] = fn;
    if (lm[l]) {
      const double e = exp(fn - f_old[l]);
      se += e;
      se2 += e * e;
    }
  }
  se = block_sum_f64(se, sh);
  se2 = block_sum_f64(se2, sh);
  if (threadIdx.x == 0) { parts[2 * blockIdx.x] = se; parts[2 * blockIdx.x + 1] = se2; }
}

// ---- apply: rows of the volume -----------------------------------------------------------------------------------------------------
// A workgroup owns `rows` consecutive rows (one z, consecutive y) of a run of at most N4_XRUN voxels along x, about 4096 voxels.  It
// first writes into LDS the cell and the four weights of every x of its run and of every y of its rows -- per row and per column, not
// per voxel: the five fp64 divisions of n4_basis are paid once per line -- and per row the 4 x 4 control points over (z, y) combined
// into the M2 + 3 coefficients of a one-dimensional spline along x.  A voxel then costs four multiply-adds, one exp and one division.
// x is read once and out written once: 8 bytes per voxel (12 with the field).
__global__ __launch_bounds__(256) void n4_apply_kernel(const float* __restrict__ x, const double* __restrict__ phi, const N4Geo g, int rows,
                                                       float* __restrict__ out, float* __restrict__ field) {
  __shared__ double co[N4_ROWS][N4_MAXMESH + 3];
  __shared__ double wx[N4_XRUN][4], wy[N4_ROWS][4];
  __shared__ int ix[N4_XRUN], iy[N4_ROWS];
  const int P1 = g.M[1] + 3, P2 = g.M[2] + 3, W = g.N[2];
  const int runs = (W + N4_XRUN - 1) / N4_XRUN, groups = (g.N[1] + rows - 1) / rows;
  const int run = (int)(blockIdx.x % runs), grp = (int)(blockIdx.x / runs % groups), z = (int)(blockIdx.x / runs / groups);
  const int y0 = grp * rows, x0 = run * N4_XRUN;
  const int nrows = min(rows, g.N[1] - y0), nx = min(N4_XRUN, W - x0);
  for (int e = threadIdx.x; e < nx + nrows; e += 256) {
    double w[4];
    if (e < nx) {
      ix[e] = n4_basis(x0 + e, W, g.M[2], w);
      wx[e][0] = w[0]; wx[e][1] = w[1]; wx[e][2] = w[2]; wx[e][3] = w[3];
    } else {
      const int rr = e - nx;
      iy[rr] = n4_basis(y0 + rr, g.N[1], g.M[1], w);
      wy[rr][0] = w[0]; wy[rr][1] = w[1]; wy[rr][2] = w[2]; wy[rr][3] = w[3];
    }
  }
  double w0[4];
  const int i0 = n4_basis(z, g.N[0], g.M[0], w0);
  __syncthreads();
  for (int e = threadIdx.x; e < nrows * P2; e += 256) {
    const int rr = e / P2, k = e % P2;
    const double* w1 = wy[rr];
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double* p = phi + ((long)(i0 + a) * P1 + iy[rr]) * P2 + k;
      const double ra = ((w1[0] * p[0] + w1[1] * p[P2]) + w1[2] * p[2 * P2]) + w1[3] * p[3 * P2];
      acc = acc + w0[a] * ra;
    }
    co[rr][k] = acc;
  }
  __syncthreads();
  const long origin = ((long)z * g.N[1] + y0) * W + x0;
  for (int e = threadIdx.x; e < nrows * nx; e += 256) {
    const int rr = e / nx, xx = e % nx;
    const double* c = co[rr] + ix[xx];
    const double* w2 = wx[xx];
    const double fv = ((w2[0] * c[0] + w2[1] * c[1]) + w2[2] * c[2]) + w2[3] * c[3];
    const double b = exp(fv);
    const long at = origin + (long)rr * W + xx;
    out[at] = (float)((double)x[at] / b);
    if (field != nullptr) field[at] = (float)b;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static bool n4_geo(N4Geo* g, int D, int H, int W, int s0, int s1, int s2, int M0, int M1, int M2) {
  const int N[3] = {D, H, W}, s[3] = {s0, s1, s2}, M[3] = {M0, M1, M2};
  if (D < 1 || H < 1 || W < 1 || (long)D * H * W > 0x7fffffffL) return false;
  for (int a = 0; a < 3; ++a) {
    if (s[a] < 1 || s[a] > N[a] || M[a] < 1 || M[a] > N4_MAXMESH) return false;
    g->N[a] = N[a];
    g->s[a] = s[a];
    g->o[a] = s[a] / 2;
    g->n[a] = (N[a] - 1 - g->o[a]) / s[a] + 1;
    g->M[a] = M[a];
  }
  return true;
}

extern "C" int bts_n4_log_lattice(const float* x, const uint8_t* mask_or_null, int D, int H, int W, int s0, int s1, int s2, double* v,
                                  uint8_t* lmask, hipStream_t stream) {
  N4Geo g;
  if (!n4_geo(&g, D, H, W, s0, s1, s2, 1, 1, 1)) return BTS_ERR_SHAPE;
  if (x == nullptr || v == nullptr || lmask == nullptr) return BTS_ERR_SHAPE;
  const long npts = (long)g.n[0] * g.n[1] * g.n[2];
  (void)hipGetLastError();
  hipLaunchKernelGGL(n4_log_kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, stream, x, mask_or_null, g, v, lmask, npts);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_n4_range_hist(const double* v, const double* f, const uint8_t* lmask, long npts, int bins, double* r, double* range4,
                                 long long* hist, hipStream_t stream) {
  if (npts < 1 || npts > 0x7fffffffL || bins < 2 || bins > N4_MAXBINS) return BTS_ERR_SHAPE;
  if (v == nullptr || f == nullptr || lmask == nullptr || r == nullptr || range4 == nullptr || hist == nullptr) return BTS_ERR_SHAPE;
  unsigned long long* keys = (unsigned long long*)(range4 + 2);
  const unsigned blocks = (unsigned)((npts + N4_PTS - 1) / N4_PTS);
  (void)hipGetLastError();
  hipLaunchKernelGGL(n4_init_kernel, dim3((bins + 255) / 256), dim3(256), 0, stream, keys, hist, bins);
  BTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(n4_range_kernel, dim3(blocks), dim3(256), 0, stream, v, f, lmask, npts, r, keys);
  BTS_LAUNCH_CHECK();
  hipLaunchKernelGGL(n4_hist_kernel, dim3(blocks), dim3(256), 0, stream, r, lmask, npts, bins, keys, range4, hist);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_n4_residual(const double* r, const uint8_t* lmask, const double* E, long npts, int bins, double lo, double sl,
                               double* res, hipStream_t stream) {
  if (npts < 1 || npts > 0x7fffffffL || bins < 2 || bins > N4_MAXBINS) return BTS_ERR_SHAPE;
  if (!isfinite(lo) || !isfinite(sl) || sl < 0.0) return BTS_ERR_SHAPE;
  if (r == nullptr || lmask == nullptr || E == nullptr || res == nullptr) return BTS_ERR_SHAPE;
  (void)hipGetLastError();
  hipLaunchKernelGGL(n4_residual_kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, stream, r, lmask, E, npts, bins, lo, sl, res);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_n4_fit(const double* res, const uint8_t* lmask, int D, int H, int W, int s0, int s1, int s2, int M0, int M1, int M2,
                          double* num, double* den, double* dphi, double* phi_or_null, hipStream_t stream) {
  N4Geo g;
  if (!n4_geo(&g, D, H, W, s0, s1, s2, M0, M1, M2)) return BTS_ERR_SHAPE;
  if (g.n[0] > N4_MAXN || g.n[1] > N4_MAXN || g.n[2] > N4_MAXN) return BTS_ERR_SHAPE;
  if (res == nullptr || lmask == nullptr || num == nullptr || den == nullptr || dphi == nullptr) return BTS_ERR_SHAPE;
  const unsigned cps = (unsigned)((M0 + 3) * (M1 + 3) * (M2 + 3));   // <= 67^3
  (void)hipGetLastError();
  hipLaunchKernelGGL(n4_fit_kernel, dim3(cps), dim3(256), 0, stream, res, lmask, g, num, den, dphi, phi_or_null);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" long bts_n4_eval_parts(long npts) {
  if (npts < 1 || npts > 0x7fffffffL) return -1;
  return (npts + N4_PTS - 1) / N4_PTS;
}

extern "C" int bts_n4_eval(const double* phi, int D, int H, int W, int s0, int s1, int s2, int M0, int M1, int M2, const double* f_old,
                           const uint8_t* lmask, double* f_new, double* parts, hipStream_t stream) {
  N4Geo g;
  if (!n4_geo(&g, D, H, W, s0, s1, s2, M0, M1, M2)) return BTS_ERR_SHAPE;
  if (phi == nullptr || f_old == nullptr || lmask == nullptr || f_new == nullptr || parts == nullptr) return BTS_ERR_SHAPE;
  const long npts = (long)g.n[0] * g.n[1] * g.n[2];
  (void)hipGetLastError();
  hipLaunchKernelGGL(n4_eval_kernel, dim3((unsigned)((npts + N4_PTS - 1) / N4_PTS)), dim3(256), 0, stream, phi, g, f_old, lmask, npts, f_new,
                     parts);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_n4_apply(const float* x, int D, int H, int W, const double* phi, int M0, int M1, int M2, float* out,
                            float* field_or_null, hipStream_t stream) {
  N4Geo g;
  if (!n4_geo(&g, D, H, W, 1, 1, 1, M0, M1, M2)) return BTS_ERR_SHAPE;
  if (x == nullptr || phi == nullptr || out == nullptr) return BTS_ERR_SHAPE;
  int rows = 4096 / (W < N4_XRUN ? W : N4_XRUN);
  rows = rows < 1 ? 1 : (rows > N4_ROWS ? N4_ROWS : rows);
  rows = rows > H ? H : rows;
  const long blocks = (long)D * ((H + rows - 1) / rows) * ((W + N4_XRUN - 1) / N4_XRUN);   // <= D * H * W < 2^31
  (void)hipGetLastError();
  hipLaunchKernelGGL(n4_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, phi, g, rows, out, field_or_null);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
