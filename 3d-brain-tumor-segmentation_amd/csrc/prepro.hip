// GPU-side dataset preprocessing (reference preprocess.py:17-131, numpy on the host).
// Three streaming passes over dense fp32 (S0,S1,S2,C) volumes, C innermost, 1 <= C <= 16:
//   occupancy  which planes of each axis hold an x != 0 (the bounding box of preprocess.py:39-49)
//   sums       fp64 sum of x and count of x > 0, or sum of (x - mean)^2, per channel over a crop window (preprocess.py:68-85)
//   crop_norm  float((double(x) - mean) / std) of the window and its labels with >= 4 -> 3 (preprocess.py:36,55-56,124)
// A crop window is addressed in place: pointer to its origin, element strides st0 / st1 of the two outer axes, voxel stride C.
#include "common.h"
#include "bts_internal.h"

#define PRE_MAXC 16          // AUG_MAXC of augment.hip
#define PRE_BLOCKS 1024      // partial sums of bts_prepro_sums: 4 workgroups per CU
#define PRE_ROWS 8           // (i0,i1) rows per workgroup visit
#define OCC_COLS 4096        // axis-2 planes one workgroup flags in LDS; longer rows take gridDim.y column tiles
#define PRE_MAXWG (1L << 24) // a launch holds fewer than 2^32 threads: fewer than 2^24 workgroups of 256

// ---- occupancy -------------------------------------------------------------------------------------------------------------
// One workgroup per batch of PRE_ROWS rows and tile of OCC_COLS columns.  Flags are gathered in LDS and flushed with plain vector
// stores of the constant 1: every writer of a word stores the same value, so the result does not depend on scheduling.
// V = floats per load (4 / 2 where every row segment is 16 / 8-byte aligned, else 1).
template <int V>
__global__ __launch_bounds__(256) void occupancy_kernel(const float* __restrict__ x, int* occ, int S0, int S1, int S2, int C) {
  __shared__ int col[OCC_COLS];
  __shared__ int rowf[PRE_ROWS];
  const long rows = (long)S0 * S1;
  const long row0 = (long)blockIdx.x * PRE_ROWS;
  const int nrow = (int)(rows - row0 < PRE_ROWS ? rows - row0 : PRE_ROWS);
  const int c0 = blockIdx.y * OCC_COLS;
  const int ncol = S2 - c0 < OCC_COLS ? S2 - c0 : OCC_COLS;
  for (int i = threadIdx.x; i < ncol; i += 256) col[i] = 0;
  if (threadIdx.x < PRE_ROWS) rowf[threadIdx.x] = 0;
  __syncthreads();
  const int L = ncol * C;                 // floats of one row segment; L % V == 0 by the choice of V
  const int Q = L / V;
  const long L2 = (long)S2 * C;
  for (int i = threadIdx.x; i < nrow * Q; i += 256) {
    const int r = i / Q, q = i - r * Q;
    const float* p = x + (row0 + r) * L2 + (long)c0 * C + (long)q * V;
    float v[V];
    if constexpr (V == 4) { const f32x4 t = *reinterpret_cast<const f32x4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else if constexpr (V == 2) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; }
    else v[0] = *p;
    bool any = false;
#pragma unroll
    for (int k = 0; k < V; ++k) any |= (v[k] != 0.f);   // NaN != 0 is true, -0.0 != 0 is false: numpy's truth value
    if (any) {
      rowf[r] = 1;
      int cc = (q * V) / C, rem = (q * V) - cc * C;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (v[k] != 0.f) col[cc] = 1;
        if (++rem == C) { rem = 0; ++cc; }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncol; i += 256)
    if (col[i]) occ[S0 + S1 + c0 + i] = 1;
  if (threadIdx.x < nrow && rowf[threadIdx.x]) {
    const long row = row0 + threadIdx.x;
    occ[(int)(row / S1)] = 1;
    occ[S0 + (int)(row % S1)] = 1;
  }
}

extern "C" int bts_prepro_occupancy(const float* x, int* occ, int S0, int S1, int S2, int C, hipStream_t stream) {
  if (S0 <= 0 || S1 <= 0 || S2 <= 0 || C <= 0 || C > PRE_MAXC) return BTS_ERR_SHAPE;
  const long rows = (long)S0 * S1;
  const long nb = (rows + PRE_ROWS - 1) / PRE_ROWS;
  const int tiles = (S2 + OCC_COLS - 1) / OCC_COLS;
  if (tiles > 65535 || nb * tiles >= PRE_MAXWG) return BTS_ERR_SHAPE;
  const dim3 grid((unsigned)nb, (unsigned)tiles), block(256);
  // every row segment starts at x + (row * S2 + tile * OCC_COLS) * C floats: aligned to V floats when S2 * C is (OCC_COLS * C is)
  const long L2 = (long)S2 * C;
  const uintptr_t a = reinterpret_cast<uintptr_t>(x);
  (void)hipGetLastError();
  if (L2 % 4 == 0 && a % 16 == 0) hipLaunchKernelGGL(occupancy_kernel<4>, grid, block, 0, stream, x, occ, S0, S1, S2, C);
  else if (L2 % 2 == 0 && a % 8 == 0) hipLaunchKernelGGL(occupancy_kernel<2>, grid, block, 0, stream, x, occ, S0, S1, S2, C);
  else hipLaunchKernelGGL(occupancy_kernel<1>, grid, block, 0, stream, x, occ, S0, S1, S2, C);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- per-channel sums over a window ------------------------------------------------------------------------------------------
// A thread owns whole voxels, so its C accumulators are registers.  Partials are fp64 per thread, one per workgroup in the workspace,
// and a fixed-order finalize adds them into acc: no float atomics, successive calls on one stream accumulate in call order.
// CT = C where a voxel is loaded in one piece (C in {1,2,4} and every voxel aligned to it), 0 = any C, scalar loads.
template <int CT>
__global__ __launch_bounds__(256) void prepro_sums_kernel(const float* __restrict__ x, long st0, long st1, int T0, int T1, int T2,
                                                          int C, const double* __restrict__ mean, double* part) {
  __shared__ double sh[4];
  constexpr int NC = CT ? CT : PRE_MAXC;
  double s[NC], m[NC];
  int cnt[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) { s[c] = 0.0; cnt[c] = 0; m[c] = (mean && c < C) ? mean[c] : 0.0; }
  const bool second = mean != nullptr;
  const long rows = (long)T0 * T1;
  const long nbatch = (rows + PRE_ROWS - 1) / PRE_ROWS;
  for (long b = blockIdx.x; b < nbatch; b += gridDim.x) {
    const long row0 = b * PRE_ROWS;
    const int nrow = (int)(rows - row0 < PRE_ROWS ? rows - row0 : PRE_ROWS);
    for (int i = threadIdx.x; i < nrow * T2; i += 256) {
      const int r = i / T2, i2 = i - r * T2;
      const long row = row0 + r;
      const float* p = x + (row / T1) * st0 + (row % T1) * st1 + (long)i2 * C;
      float v[NC];
      if constexpr (CT == 4) { const f32x4 t = *reinterpret_cast<const f32x4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
      else if constexpr (CT == 2) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; }
      else {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = (c < C) ? p[c] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < C) {
          if (second) { const double d = (double)v[c] - m[c]; s[c] += d * d; }
          else { s[c] += (double)v[c]; cnt[c] += (v[c] > 0.f) ? 1 : 0; }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < C) {
      const double a = block_sum_f64(s[c], sh);
      const double n = block_sum_f64((double)cnt[c], sh);   // < 2^31 per thread, < 2^53 in all: exact
      if (threadIdx.x == 0) { part[(long)blockIdx.x * 2 * C + c] = a; part[(long)blockIdx.x * 2 * C + C + c] = n; }
    }
  }
}
// one wave per output: lane l adds partials l, l+64, ... in order, then the fixed-order wave sum; acc[k] += total
__global__ __launch_bounds__(64) void prepro_sums_finalize_kernel(const double* part, double* acc, int nblocks, int C) {
  const int k = blockIdx.x;   // 0..C-1 sums, C..2C-1 counts
  double t = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) t += part[(long)b * 2 * C + k];
  t = wave_sum_f64(t);
  if (threadIdx.x == 0) acc[k] += t;
}

extern "C" long bts_prepro_workspace(int C) {
  if (C <= 0 || C > PRE_MAXC) return -1;
  return (long)PRE_BLOCKS * 2 * C * sizeof(double);
}

static bool window_ok(long st0, long st1, int T0, int T1, int T2, int ld) {
  return T0 > 0 && T1 > 0 && T2 > 0 && st1 >= (long)T2 * ld && st0 >= (long)T1 * st1;
}

extern "C" int bts_prepro_sums(const float* xwin, long st0, long st1, int T0, int T1, int T2, int C, const double* mean_or_null,
                               double* acc, void* workspace, long workspace_bytes, hipStream_t stream) {
  if (C <= 0 || C > PRE_MAXC || !window_ok(st0, st1, T0, T1, T2, C)) return BTS_ERR_SHAPE;
  if ((long)PRE_ROWS * T2 > 0x7fffffffL) return BTS_ERR_SHAPE;
  if (workspace == nullptr || workspace_bytes < bts_prepro_workspace(C)) return BTS_ERR_WORKSPACE;
  const long nbatch = ((long)T0 * T1 + PRE_ROWS - 1) / PRE_ROWS;
  const int blocks = (int)(nbatch < PRE_BLOCKS ? nbatch : PRE_BLOCKS);
  double* part = reinterpret_cast<double*>(workspace);
  // a voxel is one aligned load where the window origin and both strides are multiples of C floats of C * 4 bytes
  const uintptr_t a = reinterpret_cast<uintptr_t>(xwin);
  const bool vec = (C == 4 || C == 2) && a % (C * 4) == 0 && st0 % C == 0 && st1 % C == 0;
  (void)hipGetLastError();
  if (vec && C == 4) hipLaunchKernelGGL(prepro_sums_kernel<4>, dim3(blocks), dim3(256), 0, stream, xwin, st0, st1, T0, T1, T2, C, mean_or_null, part);
  else if (vec && C == 2) hipLaunchKernelGGL(prepro_sums_kernel<2>, dim3(blocks), dim3(256), 0, stream, xwin, st0, st1, T0, T1, T2, C, mean_or_null, part);
  else if (C == 1) hipLaunchKernelGGL(prepro_sums_kernel<1>, dim3(blocks), dim3(256), 0, stream, xwin, st0, st1, T0, T1, T2, C, mean_or_null, part);
  else hipLaunchKernelGGL(prepro_sums_kernel<0>, dim3(blocks), dim3(256), 0, stream, xwin, st0, st1, T0, T1, T2, C, mean_or_null, part);
  BTS_LAUNCH_CHECK();
  (void)hipGetLastError();
  hipLaunchKernelGGL(prepro_sums_finalize_kernel, dim3(mean_or_null ? C : 2 * C), dim3(64), 0, stream, part, acc, blocks, C);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- crop + normalise + label rule, one pass ----------------------------------------------------------------------------------
// An item is four consecutive floats of one row (of x: T2*C floats, of y: T2).  It moves as one 16-byte load and one 16-byte store
// where both addresses are 16-byte aligned and the row holds all four, and float by float where not (a window origin with odd
// lo2*C, the tail of a row).  IEEE fp64 subtract and divide, one rounding to fp32: the value numpy's float64 expression stores.
__device__ __forceinline__ float norm1(float v, double m, double s) { return (float)(((double)v - m) / s); }
__device__ __forceinline__ float label1(float v) { return v >= 4.f ? 3.f : v; }

__global__ __launch_bounds__(256) void crop_norm_kernel(const float* __restrict__ x, const float* __restrict__ y, long st0, long st1,
                                                        long yst0, long yst1, int T0, int T1, int T2, int C,
                                                        const double* __restrict__ mean, const double* __restrict__ stdv,
                                                        float* __restrict__ xo, float* __restrict__ yo) {
  __shared__ double sm[PRE_MAXC], ss[PRE_MAXC];
  if (threadIdx.x < C) { sm[threadIdx.x] = mean[threadIdx.x]; ss[threadIdx.x] = stdv[threadIdx.x]; }
  __syncthreads();
  const long rows = (long)T0 * T1;
  const long row0 = (long)blockIdx.x * PRE_ROWS;
  const int nrow = (int)(rows - row0 < PRE_ROWS ? rows - row0 : PRE_ROWS);
  const int L = T2 * C, Q = (L + 3) / 4;
  for (int i = threadIdx.x; i < nrow * Q; i += 256) {
    const int r = i / Q, e0 = (i - r * Q) * 4;
    const long row = row0 + r;
    const float* p = x + (row / T1) * st0 + (row % T1) * st1 + e0;
    float* o = xo + row * L + e0;
    int c = e0 % C;
    if (e0 + 4 <= L && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p);
      f32x4 w;
      w.x = norm1(t.x, sm[c], ss[c]); if (++c == C) c = 0;
      w.y = norm1(t.y, sm[c], ss[c]); if (++c == C) c = 0;
      w.z = norm1(t.z, sm[c], ss[c]); if (++c == C) c = 0;
      w.w = norm1(t.w, sm[c], ss[c]);
      *reinterpret_cast<f32x4*>(o) = w;
    } else {
      const int n = L - e0 < 4 ? L - e0 : 4;
      for (int k = 0; k < n; ++k) { o[k] = norm1(p[k], sm[c], ss[c]); if (++c == C) c = 0; }
    }
  }
  if (y == nullptr) return;
  const int Qy = (T2 + 3) / 4;
  for (int i = threadIdx.x; i < nrow * Qy; i += 256) {
    const int r = i / Qy, e0 = (i - r * Qy) * 4;
    const long row = row0 + r;
    const float* p = y + (row / T1) * yst0 + (row % T1) * yst1 + e0;
    float* o = yo + row * T2 + e0;
    if (e0 + 4 <= T2 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p);
      f32x4 w;
      w.x = label1(t.x); w.y = label1(t.y); w.z = label1(t.z); w.w = label1(t.w);
      *reinterpret_cast<f32x4*>(o) = w;
    } else {
      const int n = T2 - e0 < 4 ? T2 - e0 : 4;
      for (int k = 0; k < n; ++k) o[k] = label1(p[k]);
    }
  }
}

extern "C" int bts_prepro_crop_norm(const float* xwin, const float* ywin, long st0, long st1, long yst0, long yst1, int T0, int T1,
                                    int T2, int C, const double* mean, const double* stdv, float* xo, float* yo,
                                    hipStream_t stream) {
  if (C <= 0 || C > PRE_MAXC || !window_ok(st0, st1, T0, T1, T2, C)) return BTS_ERR_SHAPE;
  if (ywin != nullptr && !window_ok(yst0, yst1, T0, T1, T2, 1)) return BTS_ERR_SHAPE;
  if ((long)PRE_ROWS * ((long)T2 * C + 3) > 0x7fffffffL) return BTS_ERR_SHAPE;
  const long nb = ((long)T0 * T1 + PRE_ROWS - 1) / PRE_ROWS;
  if (nb >= PRE_MAXWG) return BTS_ERR_SHAPE;
  (void)hipGetLastError();
  hipLaunchKernelGGL(crop_norm_kernel, dim3((unsigned)nb), dim3(256), 0, stream, xwin, ywin, st0, st1, yst0, yst1, T0, T1, T2, C,
                     mean, stdv, xo, yo);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
