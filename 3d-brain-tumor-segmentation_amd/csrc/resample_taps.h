// Tap arithmetic shared by the two resampling kernels (resample.hip: bts_zoom3d on zoom()'s per-axis grid; conform.hip:
// bts_affine_resample3d on a general affine grid): the reflect rule, the tap indices and fp32 weights of orders 0 / 1 / 3, and whole-voxel
// loads and stores of C <= 8 channels.
#pragma once
#include "common.h"

#define RS_MAXC 8

// half-sample symmetric reflection (-1 -> 0, n -> n-1), then clamped so that no extent can index outside the line
__device__ __forceinline__ int rs_reflect(int i, int n) {
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - 1 - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// taps and weights of the fp64 coordinate c on an input line of n samples: the tap indices are SciPy's, the weights are fp32
template <int NT>
__device__ __forceinline__ void rs_taps_at(const double c, int n, int* idx, float* wt) {
  if constexpr (NT == 1) {
    idx[0] = rs_reflect((int)floor(c + 0.5), n);
    wt[0] = 1.f;
  } else {
    const double fl = floor(c);
    const int i0 = (int)fl;
    const float t = (float)(c - fl);
    if constexpr (NT == 2) {
      idx[0] = rs_reflect(i0, n); idx[1] = rs_reflect(i0 + 1, n);
      wt[0] = 1.f - t; wt[1] = 1.f - wt[0];  // zoom() forms the last weight as 1 - the others
    } else {
      const float u = 1.f - t;
      wt[1] = (t * t * (t - 2.f) * 3.f + 4.f) / 6.f;
      wt[2] = (u * u * (u - 2.f) * 3.f + 4.f) / 6.f;
      wt[0] = u * u * u / 6.f;
      wt[3] = 1.f - wt[0] - wt[1] - wt[2];
#pragma unroll
      for (int k = 0; k < 4; ++k) idx[k] = rs_reflect(i0 - 1 + k, n);
    }
  }
}

// taps and weights of output index o of zoom(): the coordinate o * scale is formed in fp64 as zoom() does
template <int NT>
__device__ __forceinline__ void rs_taps(int o, double scale, int n, int* idx, float* wt) {
  rs_taps_at<NT>((double)o * scale, n, idx, wt);
}

template <int C>
__device__ __forceinline__ void rs_load(const float* p, float* v) {
  if (C % 4 == 0) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
      const float4 t = reinterpret_cast<const float4*>(p)[q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  } else if (C == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[c];
  }
}
template <int C>
__device__ __forceinline__ void rs_store(float* p, const float* v) {
  if (C % 4 == 0) {
#pragma unroll
    for (int q = 0; q < C / 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else if (C == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = v[c];
  }
}

// acc[c] = the NT^3 taps of a dense (.,Hin,Win,C) volume.  Order 1 sums its 8 taps as zoom() does, ((v * wd) * wh) * ww in row-major tap
// order; order 3 sums separably, W innermost; order 0 is the one sample.  This is the tap loop of rs_zoom_kernel, which keeps it in its own
// body: moved out, the compiler schedules that kernel differently, and its code is the measured one.
template <int C, int NT>
__device__ __forceinline__ void rs_accumulate(const float* coef, int Hin, int Win, const int* id, const int* ih, const int* iw,
                                              const float* wd, const float* wh, const float* ww, float* acc) {
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    float ah[C];
#pragma unroll
    for (int c = 0; c < C; ++c) ah[c] = 0.f;
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const float* row = coef + ((long)id[a] * Hin + ih[b]) * Win * C;
      float aw[C];
#pragma unroll
      for (int c = 0; c < C; ++c) aw[c] = 0.f;
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        float t[C];
        rs_load<C>(row + (long)iw[k] * C, t);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if (NT == 1) acc[c] = t[c];
          else if (NT == 2) acc[c] += ((t[c] * wd[a]) * wh[b]) * ww[k];
          else aw[c] += ww[k] * t[c];
        }
      }
      if (NT == 4) {
#pragma unroll
        for (int c = 0; c < C; ++c) ah[c] += wh[b] * aw[c];
      }
    }
    if (NT == 4) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += wd[a] * ah[c];
    }
  }
}
