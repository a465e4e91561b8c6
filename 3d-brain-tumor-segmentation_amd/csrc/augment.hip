// GPU-side training augmentation (reference train.py:14-49, a tf.data map on the host).
// Per example: per-channel intensity shift/scale driven by the volume's per-channel standard deviation, a random
// crop_size window of the (x,y) pair, per-axis flips, and one-hot labels without the background channel.
// The random draws are arguments (the TF stream cannot be reproduced); given the draws the arithmetic is the
// reference's: x <- (x + shift*sqrt(var)) * scale in fp32, var = population variance over the whole volume.
#include <cmath>
#include "common.h"
#include "bts_internal.h"

#define AUG_MAXC 16
#define AUG_BLOCKS 512

// per-block fp64 partial sums of d and d^2, d = x - pivot[c] with pivot = the first voxel's value, for every channel; combined in a
// fixed order by the finalize kernel.  Shifted because E[x^2] - mean^2 on raw intensities (mean 1000, deviation 1) cancels six digits
// of the fp64 sums, and a constant volume came out with a variance of +-1e-8 instead of 0; on d a constant volume sums exact zeros.
__global__ __launch_bounds__(256) void moments_partial_kernel(const float* __restrict__ x, double* part, long nvox, int C,
                                                              int ld) {
  __shared__ double sh[4];
  double s[AUG_MAXC], q[AUG_MAXC];
#pragma unroll
  for (int c = 0; c < AUG_MAXC; ++c) { s[c] = 0.0; q[c] = 0.0; }
  double pv[AUG_MAXC];
#pragma unroll
  for (int c = 0; c < AUG_MAXC; ++c) pv[c] = (c < C) ? (double)x[c] : 0.0;
  for (long v = blockIdx.x * (long)blockDim.x + threadIdx.x; v < nvox; v += (long)gridDim.x * blockDim.x) {
    const float* row = x + v * ld;
#pragma unroll
    for (int c = 0; c < AUG_MAXC; ++c)
      if (c < C) { const double t = (double)row[c] - pv[c]; s[c] += t; q[c] += t * t; }
  }
#pragma unroll
  for (int c = 0; c < AUG_MAXC; ++c) {
    if (c < C) {
      const double a = block_sum_f64(s[c], sh);
      const double b = block_sum_f64(q[c], sh);
      if (threadIdx.x == 0) { part[((long)blockIdx.x * C + c) * 2 + 0] = a; part[((long)blockIdx.x * C + c) * 2 + 1] = b; }
    }
  }
}
__global__ void moments_finalize_kernel(const float* __restrict__ x, const double* part, float* mean, float* var, int nblocks, int C,
                                        long nvox) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < nblocks; ++b) { s += part[((long)b * C + c) * 2 + 0]; q += part[((long)b * C + c) * 2 + 1]; }
  const double m = s / (double)nvox;      // mean of x - pivot
  double vv = q / (double)nvox - m * m;  // population variance (tf.nn.moments); a shift leaves it unchanged
  if (vv < 0.0) vv = 0.0;
  if (mean) mean[c] = (float)((double)x[c] + m);
  var[c] = (float)vv;
}

extern "C" long bts_channel_moments_workspace(int C) { return (long)AUG_BLOCKS * C * 2 * sizeof(double); }

extern "C" int bts_channel_moments(const float* x, float* mean, float* var, void* workspace, long workspace_bytes, long nvox,
                                   int C, int ld, hipStream_t stream) {
  if (nvox <= 0 || C <= 0 || C > AUG_MAXC || ld < C) return BTS_ERR_SHAPE;
  if (workspace == nullptr || workspace_bytes < bts_channel_moments_workspace(C)) return BTS_ERR_WORKSPACE;
  long blocks = (nvox + 255) / 256;
  if (blocks > AUG_BLOCKS) blocks = AUG_BLOCKS;
  double* part = reinterpret_cast<double*>(workspace);
  (void)hipGetLastError(); hipLaunchKernelGGL(moments_partial_kernel, dim3((int)blocks), dim3(256), 0, stream, x, part, nvox, C, ld);
  BTS_LAUNCH_CHECK();
  (void)hipGetLastError(); hipLaunchKernelGGL(moments_finalize_kernel, dim3(1), dim3(64), 0, stream, x, part, mean, var, (int)blocks, C, nvox);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- crop + flips + intensity shift/scale + one-hot of a whole batch in one launch ----
// The table of the examples travels by value in the kernel arguments (4 KB at the most: 72 B of header + 16 entries of 176 B).
#define AUG_BATCH_MAX 16
struct AugEntry {
  const float* x;    // (S0,S1,S2,C) source volume
  const float* y;    // (S0,S1,S2) labels stored as floats
  const float* var;  // C: per-channel population variance of the source volume
  int o0, o1, o2, flip;
  int xvec, pad;     // floats per access of the channels_last x pass (4, 2 or 1): what C and the alignment of this example's rows allow
  float shift[AUG_MAXC], scale[AUG_MAXC];
};
struct AugBatch {
  float* xo;         // layout 0: (n,T0,T1,T2,C)       layout 1: (n,C,T0,T1,T2)
  float* yo;         // layout 0: (n,T0,T1,T2,out_ch)  layout 1: (n,out_ch,T0,T1,T2)
  int S0, S1, S2, C, T0, T1, T2, out_ch, layout, n;
  int chunks, rows;  // a work unit is `rows` consecutive crop rows of one (example, t0) plane; `chunks` units per plane
  int xgroup, ygroup;  // 1: xo (layout 1) / yo rows take 16-byte stores of four voxels
  AugEntry e[AUG_BATCH_MAX];
};

// train.py:19-22 (x += shift * sqrt(var); x *= scale): one fused multiply-add on the correctly rounded root, then the product
__device__ __forceinline__ float aug_value(float v, float shift, float sd, float scale) { return __builtin_fmaf(shift, sd, v) * scale; }

template <int V> __device__ __forceinline__ void aug_ld(const float* p, float (&r)[V]) {
  if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; }
  else if constexpr (V == 2) { const float2 t = *reinterpret_cast<const float2*>(p); r[0] = t.x; r[1] = t.y; }
  else r[0] = *p;
}
template <int V> __device__ __forceinline__ void aug_st(float* p, const float (&r)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
  else if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
  else *p = r[0];
}

// how the 64 lanes of a wave share rows of `items` work items: L = 2^l lanes per row (the smallest power of two >= items, 64 at the
// most), 64 / L rows per wave
struct AugLanes { int first, step, sub, per_wave; };
__device__ __forceinline__ AugLanes aug_lanes(int items, int lane) {
  int l = 0;
  while ((1 << l) < items && l < 6) ++l;
  AugLanes a;
  a.first = lane & ((1 << l) - 1); a.step = 1 << l; a.sub = lane >> l; a.per_wave = 64 >> l;
  return a;
}

// channels_last x row, C < V (C = 1 or 2 divides V): a lane moves V floats = V / C whole voxels; under an axis-2 flip the voxels are
// reversed inside the access and between accesses, the channels of a voxel are not
template <int V> __device__ __forceinline__ void aug_x_row_packed(const float* s, float* d, int nvec, int C, bool flip, int first, int step,
                                                                  const float* co) {
  const float sh0 = co[0], sd0 = co[AUG_MAXC], sc0 = co[2 * AUG_MAXC];
  const int c1 = C - 1;      // 0 or 1
  const float sh1 = co[c1], sd1 = co[AUG_MAXC + c1], sc1 = co[2 * AUG_MAXC + c1];
  for (int u = first; u < nvec; u += step) {
    float r[V], o[V];
    aug_ld<V>(s + (long)(flip ? nvec - 1 - u : u) * V, r);
    if (flip) {
      if (C == 1) {
#pragma unroll
        for (int k = 0; k < V / 2; ++k) { const float t = r[k]; r[k] = r[V - 1 - k]; r[V - 1 - k] = t; }
      } else if constexpr (V == 4) {
        float t = r[0]; r[0] = r[2]; r[2] = t;
        t = r[1]; r[1] = r[3]; r[3] = t;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = (k & 1) ? aug_value(r[k], sh1, sd1, sc1) : aug_value(r[k], sh0, sd0, sc0);
    aug_st<V>(d + (long)u * V, o);
  }
}
// channels_last x row, V divides C: a lane moves one voxel, V floats per access
template <int V> __device__ __forceinline__ void aug_x_row_voxel(const float* s, float* d, int T2, int C, bool flip, int first, int step,
                                                                 const float* co) {
  for (int t2 = first; t2 < T2; t2 += step) {
    const float* sv = s + (long)(flip ? T2 - 1 - t2 : t2) * C;
    float* dv = d + (long)t2 * C;
    for (int c = 0; c < C; c += V) {
      float r[V], o[V];
      aug_ld<V>(sv + c, r);
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = aug_value(r[k], co[c + k], co[AUG_MAXC + c + k], co[2 * AUG_MAXC + c + k]);
      aug_st<V>(dv + c, o);
    }
  }
}
// channels_last label row, four voxels per lane: 4 * OC floats of one-hot values as OC 16-byte stores
template <int OC> __device__ __forceinline__ void aug_y_row_group(const float* s, float* d, int T2, bool flip, int first, int step) {
  for (int g = first; g < T2 / 4; g += step) {
    int lbl[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) lbl[e] = (int)s[flip ? T2 - 1 - (4 * g + e) : 4 * g + e];     // tf.cast(y, tf.int32) truncates (train.py:38)
    float* dg = d + (long)g * 4 * OC;
#pragma unroll
    for (int m = 0; m < OC; ++m) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { const int f = 4 * m + e; o[e] = (lbl[f / OC] == f % OC + 1) ? 1.f : 0.f; }
      aug_st<4>(dg + 4 * m, o);
    }
  }
}

// A block of four waves takes work units (example, t0, chunk of rows) in a grid-stride loop; all index arithmetic is per unit and per
// row, a lane only steps along its row.  Every output element is written once; nothing outside the crop windows is read.
__global__ __launch_bounds__(256) void augment_batch_kernel(const AugBatch p) {
  __shared__ float co[3 * AUG_MAXC];      // shift | sqrt(var) | scale of the unit's example
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = p.C, T0 = p.T0, T1 = p.T1, T2 = p.T2, OC = p.out_ch;
  const long plane = (long)T1 * T2, vol = (long)T0 * plane;
  const int units = p.n * T0 * p.chunks;
  for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int chunk = unit % p.chunks, t = unit / p.chunks, t0 = t % T0, n = t / T0;
    const AugEntry& e = p.e[n];
    __syncthreads();        // (the previous unit's readers of co are done)
    if ((int)threadIdx.x < C) {
      co[threadIdx.x] = e.shift[threadIdx.x];
      co[AUG_MAXC + threadIdx.x] = sqrtf(e.var[threadIdx.x]);
      co[2 * AUG_MAXC + threadIdx.x] = e.scale[threadIdx.x];
    }
    __syncthreads();
    const int r0 = chunk * p.rows, r1 = min(T1, r0 + p.rows);
    const int s0 = e.o0 + ((e.flip & 4) ? T0 - 1 - t0 : t0);
    const bool f1 = e.flip & 2, f2 = e.flip & 1;
    const float* xs = e.x;
    const float* ys = e.y;
    // ---- x ----
    if (p.layout == 0) {
      const int V = e.xvec;
      const bool packed = C < V;
      const AugLanes a = aug_lanes(packed ? T2 * C / V : T2, lane);
      for (int t1 = r0 + wave * a.per_wave + a.sub; t1 < r1; t1 += 4 * a.per_wave) {
        const long srow = ((long)s0 * p.S1 + (e.o1 + (f1 ? T1 - 1 - t1 : t1))) * p.S2 + e.o2;
        const float* s = xs + srow * C;
        float* d = p.xo + ((long)n * vol + (long)t0 * plane + (long)t1 * T2) * C;
        if (packed) {
          if (V == 4) aug_x_row_packed<4>(s, d, T2 * C / 4, C, f2, a.first, a.step, co);
          else aug_x_row_packed<2>(s, d, T2 * C / 2, C, f2, a.first, a.step, co);
        } else if (V == 4) aug_x_row_voxel<4>(s, d, T2, C, f2, a.first, a.step, co);
        else if (V == 2) aug_x_row_voxel<2>(s, d, T2, C, f2, a.first, a.step, co);
        else aug_x_row_voxel<1>(s, d, T2, C, f2, a.first, a.step, co);
      }
    } else {
      // channels first: a lane gathers four (or one) voxels of a channel at the source's stride C and stores them side by side
      const int G = p.xgroup ? 4 : 1;
      const AugLanes a = aug_lanes(T2 / G, lane);
      for (int t1 = r0 + wave * a.per_wave + a.sub; t1 < r1; t1 += 4 * a.per_wave) {
        const long srow = ((long)s0 * p.S1 + (e.o1 + (f1 ? T1 - 1 - t1 : t1))) * p.S2 + e.o2;
        const float* s = xs + srow * C;
        float* d = p.xo + (long)n * C * vol + (long)t0 * plane + (long)t1 * T2;
        for (int g = a.first; g < T2 / G; g += a.step) {
          for (int c = 0; c < C; ++c) {
            const float sh = co[c], sd = co[AUG_MAXC + c], sc = co[2 * AUG_MAXC + c];
            if (G == 4) {
              float o[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) o[k] = aug_value(s[(long)(f2 ? T2 - 1 - (4 * g + k) : 4 * g + k) * C + c], sh, sd, sc);
              aug_st<4>(d + c * vol + 4 * g, o);
            } else {
              d[c * vol + g] = aug_value(s[(long)(f2 ? T2 - 1 - g : g) * C + c], sh, sd, sc);
            }
          }
        }
      }
    }
    // ---- labels: one_hot(out_ch + 1) minus channel 0 (train.py:41-43) ----
    const bool grouped = p.ygroup != 0 && (p.layout == 1 || OC <= 4);
    const int G = grouped ? 4 : 1;
    const AugLanes a = aug_lanes(T2 / G, lane);
    for (int t1 = r0 + wave * a.per_wave + a.sub; t1 < r1; t1 += 4 * a.per_wave) {
      const long srow = ((long)s0 * p.S1 + (e.o1 + (f1 ? T1 - 1 - t1 : t1))) * p.S2 + e.o2;
      const float* s = ys + srow;
      const long orow = (long)t0 * plane + (long)t1 * T2;
      if (p.layout == 0) {
        float* d = p.yo + ((long)n * vol + orow) * OC;
        if (grouped) {
          if (OC == 1) aug_y_row_group<1>(s, d, T2, f2, a.first, a.step);
          else if (OC == 2) aug_y_row_group<2>(s, d, T2, f2, a.first, a.step);
          else if (OC == 3) aug_y_row_group<3>(s, d, T2, f2, a.first, a.step);
          else aug_y_row_group<4>(s, d, T2, f2, a.first, a.step);
        } else {
          for (int t2 = a.first; t2 < T2; t2 += a.step) {
            const int lbl = (int)s[f2 ? T2 - 1 - t2 : t2];
            for (int k = 0; k < OC; ++k) d[(long)t2 * OC + k] = (lbl == k + 1) ? 1.f : 0.f;
          }
        }
      } else {
        float* d = p.yo + (long)n * OC * vol + orow;
        for (int g = a.first; g < T2 / G; g += a.step) {
          if (grouped) {
            int lbl[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) lbl[k] = (int)s[f2 ? T2 - 1 - (4 * g + k) : 4 * g + k];
            for (int k = 0; k < OC; ++k) {
              float o[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) o[q] = (lbl[q] == k + 1) ? 1.f : 0.f;
              aug_st<4>(d + k * vol + 4 * g, o);
            }
          } else {
            const int lbl = (int)s[f2 ? T2 - 1 - g : g];
            for (int k = 0; k < OC; ++k) d[k * vol + g] = (lbl == k + 1) ? 1.f : 0.f;
          }
        }
      }
    }
  }
}

extern "C" long bts_augment_batch_max(void) { return AUG_BATCH_MAX; }

static bool aug_aligned(const void* p, int floats) { return reinterpret_cast<uintptr_t>(p) % (sizeof(float) * floats) == 0; }

// widest access of the channels_last x pass for one example: V floats must hold whole voxels or be a whole part of one, and every
// row of the window and of the output must start on a multiple of V floats
static int aug_xvec(const float* x, const float* xo, int S2, int C, int T2, int o2) {
  for (int v = 4; v > 1; v >>= 1) {
    if (!aug_aligned(x, v) || !aug_aligned(xo, v)) continue;
    if (C % v == 0) return v;
    if (v % C == 0 && (T2 * C) % v == 0 && (S2 * C) % v == 0 && (o2 * C) % v == 0) return v;
  }
  return 1;
}

extern "C" int bts_augment_batch(const float* const* x, const float* const* y, const float* const* var, float* xo, float* yo, int N,
                                 int S0, int S1, int S2, int C, int T0, int T1, int T2, const int* offsets, const int* flips,
                                 const float* shift, const float* scale, int out_ch, int layout, hipStream_t stream) {
  if (N <= 0 || C <= 0 || C > AUG_MAXC || out_ch <= 0 || T0 <= 0 || T1 <= 0 || T2 <= 0 || (layout != 0 && layout != 1)) return BTS_ERR_SHAPE;
  if (x == nullptr || y == nullptr || var == nullptr || offsets == nullptr || flips == nullptr || shift == nullptr || scale == nullptr)
    return BTS_ERR_SHAPE;
  for (int n = 0; n < N; ++n) {
    const int* o = offsets + 3 * n;
    if (flips[n] & ~7) return BTS_ERR_SHAPE;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0 || o[0] > S0 - T0 || o[1] > S1 - T1 || o[2] > S2 - T2) return BTS_ERR_SHAPE;
  }
  const long per_x = (long)T0 * T1 * T2 * C, per_y = (long)T0 * T1 * T2 * out_ch;
  for (int n0 = 0; n0 < N; n0 += AUG_BATCH_MAX) {
    AugBatch p;
    p.n = N - n0 < AUG_BATCH_MAX ? N - n0 : AUG_BATCH_MAX;
    p.xo = xo + n0 * per_x; p.yo = yo + n0 * per_y;
    p.S0 = S0; p.S1 = S1; p.S2 = S2; p.C = C; p.T0 = T0; p.T1 = T1; p.T2 = T2; p.out_ch = out_ch; p.layout = layout;
    // enough units to fill the chip from a small batch, whole planes once there are plenty
    const long planes = (long)p.n * T0;
    long chunks = (2048 + planes - 1) / planes;
    if (chunks > T1) chunks = T1;
    p.rows = (int)((T1 + chunks - 1) / chunks);
    p.chunks = (T1 + p.rows - 1) / p.rows;
    p.xgroup = T2 % 4 == 0 && aug_aligned(p.xo, 4);
    p.ygroup = T2 % 4 == 0 && aug_aligned(p.yo, 4);
    for (int i = 0; i < AUG_BATCH_MAX; ++i) {
      AugEntry& e = p.e[i];
      const int n = n0 + (i < p.n ? i : 0);        // (unused entries repeat the first: never read)
      e.x = x[n]; e.y = y[n]; e.var = var[n];
      e.o0 = offsets[3 * n]; e.o1 = offsets[3 * n + 1]; e.o2 = offsets[3 * n + 2]; e.flip = flips[n];
      e.xvec = aug_xvec(e.x, p.xo, S2, C, T2, e.o2); e.pad = 0;
      for (int c = 0; c < AUG_MAXC; ++c) { e.shift[c] = c < C ? shift[(long)n * C + c] : 0.f; e.scale[c] = c < C ? scale[(long)n * C + c] : 1.f; }
    }
    long blocks = planes * p.chunks;
    if (blocks > 4096) blocks = 4096;
    (void)hipGetLastError(); hipLaunchKernelGGL(augment_batch_kernel, dim3((int)blocks), dim3(256), 0, stream, p);
    BTS_LAUNCH_CHECK();
  }
  return BTS_OK;
}

// one example, channels last: the batch kernel's N = 1 call
extern "C" int bts_augment_crop(const float* x, const float* y, const float* var, float* xo, float* yo, int S0, int S1, int S2,
                                int C, int T0, int T1, int T2, int o0, int o1, int o2, int flip_mask, const float* shift,
                                const float* scale, int out_ch, hipStream_t stream) {
  const int offsets[3] = {o0, o1, o2};
  return bts_augment_batch(&x, &y, &var, xo, yo, 1, S0, S1, S2, C, T0, T1, T2, offsets, &flip_mask, shift, scale, out_ch, 0, stream);
}

// ---- the same batch launch with a spatial transform: rotation + zoom + free-form deformation, as a gather in place of the copy ----
// For an output voxel t of a crop of extent T, from a source volume of extent S at window origin o:
//   t~_k = flip_k ? T_k-1-t_k : t_k  (the flip is undone first, as in augment_batch_kernel),  q = t~ - (T-1)/2,
//   s = o + (T-1)/2 + M q + u(t~),   M = R0(th0) R1(th1) R2(th2) / z  (rotations about axes 0, 1, 2; zoom z, z > 1 magnifies; the host
//   builds M in float64 and passes 9 floats),
//   u = free-form deformation on a control grid of `spacing` voxels:  g = t~/spacing, i = floor(g), f = g - i,
//       u = sum_{a,b,c=0..3} B_a(f0) B_b(f1) B_c(f2) phi[i0+a, i1+b, i2+c, :],  B = the uniform cubic B-spline basis,
//       phi: G_k = (T_k-1)/spacing + 4 nodes per axis (integer division), 3 components, in source voxels, device memory; NULL = none.
//   Image channels: trilinear at s; a corner outside the volume contributes fill[c] (scipy's mode='grid-constant'); then
//   fmaf(shift, sqrtf(var), v) * scale on the interpolated value, var = the variance of the whole untransformed volume.
//   Labels: the nearest voxel floor(s + 0.5); outside the volume label 0; one-hot without background as above.
//   An example whose spatial flag is off is copied as augment_batch_kernel copies it (the same fmaf and product per element: bit-equal);
//   M = I with phi = NULL through the gather is bit-equal too: its coordinates are exact integers, its weights exactly 0 and 1.
// Order of the fp32 coordinate arithmetic (the tolerance of tests/test_spatial_host.py restates exactly this):
//   h_k = (T_k-1) * 0.5f, q_k = (float)t~_k - h_k, c_k = (float)o_k + h_k                       (all exact: halves of small integers)
//   m_k = fmaf(M[k][2], q2, fmaf(M[k][1], q1, M[k][0] * q0))
//   i_k = t~_k / spacing (integers), f_k = (float)(t~_k - i_k * spacing) / (float)spacing
//   B_0 = (1-f)^3 / 6, B_1 = (3 f^3 - 6 f^2 + 4) / 6, B_2 = (-3 f^3 + 3 f^2 + 3 f + 1) / 6, B_3 = f^3 / 6
//   r[c, :] = sum over a (outer), b (inner) of (B_a(f0) * B_b(f1)) * phi[i0+a, i1+b, c, :]    (per row, fmaf chain from 0, into LDS)
//   u_k = sum over c of B_c(f2) * r[i2+c, k]                                                  (fmaf chain from 0)
//   s_k = (c_k + m_k) + u_k      (+ u_k only with phi), then clamped to [-2, S_k+1] (outside that every corner is outside anyway; a NaN
//   becomes -2), j_k = floor(s_k), w_k = s_k - j_k; corner weight ((a ? w0 : 1-w0) * (b ? w1 : 1-w1)) * (c ? w2 : 1-w2), corners summed
//   in the order a, b, c = 000, 001, ..., 111 by fmaf from 0 (a voxel with all eight corners outside is fill itself, not the rounded
//   sum of its weights times fill); label voxel floor(s_k + 0.5f).
// The table entry is larger than AugEntry (304 B), so a launch carries 8 examples (the kernel arguments stay under 4 KB).
#define AUGS_BATCH_MAX 8
#define AUGS_G2MAX 256       // control nodes along axis 2 that the per-row LDS image holds
#define AUGS_PHI_LDS 3072    // floats: the four axis-0 planes of phi a unit needs are staged in LDS when they fit
struct AugSpatialEntry {
  const float* x; const float* y; const float* var;
  const float* phi;  // (G0,G1,G2,3) or NULL
  int o0, o1, o2, flip;
  int spatial, spacing, G1, G2;
  int xvec, pad;     // floats per access of a voxel's channels (4, 2 or 1)
  float M[9];
  float pad2;
  float shift[AUG_MAXC], scale[AUG_MAXC], fill[AUG_MAXC];
};
struct AugSpatialBatch {
  float* xo; float* yo;
  int S0, S1, S2, C, T0, T1, T2, out_ch, layout, n;
  int chunks, rows;
  AugSpatialEntry e[AUGS_BATCH_MAX];
};

__device__ __forceinline__ void augs_bspline(float f, float (&w)[4]) {
  const float g = 1.f - f, f2 = f * f, f3 = f2 * f;
  w[0] = g * g * g * (1.f / 6.f);
  w[1] = (3.f * f3 - 6.f * f2 + 4.f) * (1.f / 6.f);
  w[2] = (-3.f * f3 + 3.f * f2 + 3.f * f + 1.f) * (1.f / 6.f);
  w[3] = f3 * (1.f / 6.f);
}
// one axis of a sample: clamp the coordinate, split it, and give the two corner indices (clamped into the volume) with their validity
struct AugsAxis { int j[2]; bool in[2]; float w[2]; int near; bool near_in; };
__device__ __forceinline__ AugsAxis augs_axis(float s, int S) {
  s = fminf(fmaxf(s, -2.f), (float)S + 1.f);       // (fmaxf returns the other operand for a NaN)
  const float fl = floorf(s);
  const int j = (int)fl;
  AugsAxis a;
  a.w[1] = s - fl; a.w[0] = 1.f - a.w[1];
  a.in[0] = j >= 0 && j < S; a.in[1] = j + 1 >= 0 && j + 1 < S;
  a.j[0] = min(max(j, 0), S - 1); a.j[1] = min(max(j + 1, 0), S - 1);
  const int nr = (int)floorf(s + 0.5f);
  a.near_in = nr >= 0 && nr < S; a.near = min(max(nr, 0), S - 1);
  return a;
}
// the C channels of one output voxel, V floats per access; xs: the source volume, dl0: this voxel's place in a layout-0 output (or
// NULL), dl1: in a layout-1 output (channel stride vol)
template <int V> __device__ __forceinline__ void augs_x_gather(const float* xs, int S1, int S2, int C, const AugsAxis& a0,
                                                               const AugsAxis& a1, const AugsAxis& a2, const float* co, float* dl0,
                                                               float* dl1, long vol) {
  const bool any_in = (a0.in[0] || a0.in[1]) && (a1.in[0] || a1.in[1]) && (a2.in[0] || a2.in[1]);
  for (int c = 0; c < C; c += V) {
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const int a = corner >> 2, b = (corner >> 1) & 1, d = corner & 1;
      const float w = (a0.w[a] * a1.w[b]) * a2.w[d];
      const bool in = a0.in[a] && a1.in[b] && a2.in[d];
      float r[V];
      aug_ld<V>(xs + (((long)a0.j[a] * S1 + a1.j[b]) * S2 + a2.j[d]) * C + c, r);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = __builtin_fmaf(w, in ? r[k] : co[3 * AUG_MAXC + c + k], acc[k]);
    }
    float o[V];
#pragma unroll
    for (int k = 0; k < V; ++k)
      o[k] = aug_value(any_in ? acc[k] : co[3 * AUG_MAXC + c + k], co[c + k], co[AUG_MAXC + c + k], co[2 * AUG_MAXC + c + k]);
    if (dl0) aug_st<V>(dl0 + c, o);
    else {
#pragma unroll
      for (int k = 0; k < V; ++k) dl1[(c + k) * vol] = o[k];
    }
  }
}
// the copy of a voxel (spatial flag off): sv = its source voxel
template <int V> __device__ __forceinline__ void augs_x_copy(const float* sv, int C, const float* co, float* dl0, float* dl1, long vol) {
  for (int c = 0; c < C; c += V) {
    float r[V], o[V];
    aug_ld<V>(sv + c, r);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = aug_value(r[k], co[c + k], co[AUG_MAXC + c + k], co[2 * AUG_MAXC + c + k]);
    if (dl0) aug_st<V>(dl0 + c, o);
    else {
#pragma unroll
      for (int k = 0; k < V; ++k) dl1[(c + k) * vol] = o[k];
    }
  }
}

// The work unit of augment_batch_kernel: (example, t0, chunk of rows) in a grid-stride loop.  A wave takes a row, a lane steps along it.
// Every output element is written once; nothing outside the source volumes and phi is read (corner indices are clamped, fill is
// selected); no atomics: the result is deterministic.
__global__ __launch_bounds__(256) void augment_spatial_batch_kernel(const AugSpatialBatch p) {
  __shared__ float co[4 * AUG_MAXC];            // shift | sqrt(var) | scale | fill of the unit's example
  __shared__ float red[4][3 * AUGS_G2MAX];      // per wave: phi reduced over the two outer axes for the wave's row, (G2, 3)
  __shared__ float phis[AUGS_PHI_LDS];          // phi[i0 .. i0+3] of the unit
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = p.C, T0 = p.T0, T1 = p.T1, T2 = p.T2, OC = p.out_ch, S0 = p.S0, S1 = p.S1, S2 = p.S2;
  const long plane = (long)T1 * T2, vol = (long)T0 * plane;
  const int units = p.n * T0 * p.chunks;
  const float h0 = (float)(T0 - 1) * 0.5f, h1 = (float)(T1 - 1) * 0.5f, h2 = (float)(T2 - 1) * 0.5f;
  for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int chunk = unit % p.chunks, t = unit / p.chunks, t0 = t % T0, n = t / T0;
    const AugSpatialEntry& e = p.e[n];
    const int tt0 = (e.flip & 4) ? T0 - 1 - t0 : t0;
    const bool f1 = e.flip & 2, f2 = e.flip & 1;
    const bool elastic = e.spatial != 0 && e.phi != nullptr;
    const int sp = e.spacing, G1 = e.G1, G2 = e.G2;
    int i0 = 0;
    float wa[4] = {0.f, 0.f, 0.f, 0.f};
    bool staged = false;
    __syncthreads();        // (the previous unit's readers of co, red and phis are done)
    if ((int)threadIdx.x < C) {
      co[threadIdx.x] = e.shift[threadIdx.x];
      co[AUG_MAXC + threadIdx.x] = sqrtf(e.var[threadIdx.x]);
      co[2 * AUG_MAXC + threadIdx.x] = e.scale[threadIdx.x];
      co[3 * AUG_MAXC + threadIdx.x] = e.fill[threadIdx.x];
    }
    if (elastic) {
      i0 = tt0 / sp;
      augs_bspline((float)(tt0 - i0 * sp) / (float)sp, wa);
      const long slab = 4L * G1 * G2 * 3;
      staged = slab <= AUGS_PHI_LDS;
      if (staged) {
        const float* src = e.phi + (long)i0 * G1 * G2 * 3;
        for (int i = threadIdx.x; i < (int)slab; i += 256) phis[i] = src[i];
      }
    }
    __syncthreads();
    const int r0 = chunk * p.rows, r1 = min(T1, r0 + p.rows);
    const float q0 = (float)tt0 - h0;
    const float cen0 = (float)e.o0 + h0, cen1 = (float)e.o1 + h1, cen2 = (float)e.o2 + h2;
    const int V = e.xvec;
    // (the row loop is uniform over the block: its barriers order the per-wave LDS image of phi against its readers)
    for (int rb = r0; rb < r1; rb += 4) {
      const int t1 = rb + wave;
      const bool live = t1 < r1;
      const int tt1 = f1 ? T1 - 1 - t1 : t1;
      if (elastic) {
        __syncthreads();
        if (live) {
          const int i1 = tt1 / sp;
          float wb[4];
          augs_bspline((float)(tt1 - i1 * sp) / (float)sp, wb);
          for (int j = lane; j < 3 * G2; j += 64) {
            float acc = 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int b = 0; b < 4; ++b) {
                const float v = staged ? phis[((long)a * G1 + (i1 + b)) * G2 * 3 + j]
                                       : e.phi[(((long)(i0 + a)) * G1 + (i1 + b)) * G2 * 3 + j];
                acc = __builtin_fmaf(wa[a] * wb[b], v, acc);
              }
            red[wave][j] = acc;
          }
        }
        __syncthreads();
      }
      if (!live) continue;
      const long orow = (long)t0 * plane + (long)t1 * T2;
      float* xrow0 = p.layout == 0 ? p.xo + ((long)n * vol + orow) * C : nullptr;
      float* xrow1 = p.xo + (long)n * C * vol + orow;
      float* yrow = p.layout == 0 ? p.yo + ((long)n * vol + orow) * OC : p.yo + (long)n * OC * vol + orow;
      const long ystep = p.layout == 0 ? OC : 1, kstep = p.layout == 0 ? 1 : vol;
      if (e.spatial == 0) {
        const long srow = ((long)(e.o0 + tt0) * S1 + (e.o1 + tt1)) * S2 + e.o2;
        for (int t2 = lane; t2 < T2; t2 += 64) {
          const long sv = srow + (f2 ? T2 - 1 - t2 : t2);
          float* d0 = xrow0 ? xrow0 + (long)t2 * C : nullptr;
          if (V == 4) augs_x_copy<4>(e.x + sv * C, C, co, d0, xrow1 + t2, vol);
          else if (V == 2) augs_x_copy<2>(e.x + sv * C, C, co, d0, xrow1 + t2, vol);
          else augs_x_copy<1>(e.x + sv * C, C, co, d0, xrow1 + t2, vol);
          const int lbl = (int)e.y[sv];                                   // tf.cast(y, tf.int32) truncates (train.py:38)
          for (int k = 0; k < OC; ++k) yrow[t2 * ystep + k * kstep] = (lbl == k + 1) ? 1.f : 0.f;
        }
        continue;
      }
      const float q1 = (float)tt1 - h1;
      const float pre0 = __builtin_fmaf(e.M[1], q1, e.M[0] * q0), pre1 = __builtin_fmaf(e.M[4], q1, e.M[3] * q0),
                  pre2 = __builtin_fmaf(e.M[7], q1, e.M[6] * q0);
      for (int t2 = lane; t2 < T2; t2 += 64) {
        const int tt2 = f2 ? T2 - 1 - t2 : t2;
        const float q2 = (float)tt2 - h2;
        float s0 = cen0 + __builtin_fmaf(e.M[2], q2, pre0), s1 = cen1 + __builtin_fmaf(e.M[5], q2, pre1),
              s2 = cen2 + __builtin_fmaf(e.M[8], q2, pre2);
        if (elastic) {
          const int i2 = tt2 / sp;
          float wc[4];
          augs_bspline((float)(tt2 - i2 * sp) / (float)sp, wc);
          float u0 = 0.f, u1 = 0.f, u2 = 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float* r = &red[wave][(i2 + c) * 3];
            u0 = __builtin_fmaf(wc[c], r[0], u0); u1 = __builtin_fmaf(wc[c], r[1], u1); u2 = __builtin_fmaf(wc[c], r[2], u2);
          }
          s0 += u0; s1 += u1; s2 += u2;
        }
        const AugsAxis a0 = augs_axis(s0, S0), a1 = augs_axis(s1, S1), a2 = augs_axis(s2, S2);
        float* d0 = xrow0 ? xrow0 + (long)t2 * C : nullptr;
        if (V == 4) augs_x_gather<4>(e.x, S1, S2, C, a0, a1, a2, co, d0, xrow1 + t2, vol);
        else if (V == 2) augs_x_gather<2>(e.x, S1, S2, C, a0, a1, a2, co, d0, xrow1 + t2, vol);
        else augs_x_gather<1>(e.x, S1, S2, C, a0, a1, a2, co, d0, xrow1 + t2, vol);
        const bool in = a0.near_in && a1.near_in && a2.near_in;
        const float yv = e.y[((long)a0.near * S1 + a1.near) * S2 + a2.near];
        const int lbl = in ? (int)yv : 0;
        for (int k = 0; k < OC; ++k) yrow[t2 * ystep + k * kstep] = (lbl == k + 1) ? 1.f : 0.f;
      }
    }
  }
}

extern "C" long bts_augment_spatial_batch_max(void) { return AUGS_BATCH_MAX; }

extern "C" int bts_augment_spatial_batch(const float* const* x, const float* const* y, const float* const* var, float* xo, float* yo,
                                         int N, int S0, int S1, int S2, int C, int T0, int T1, int T2, const int* offsets,
                                         const int* flips, const float* shift, const float* scale, const int* spatial, const float* M,
                                         const float* const* phi, const int* spacing, const float* fill, int out_ch, int layout,
                                         hipStream_t stream) {
  if (N <= 0 || C <= 0 || C > AUG_MAXC || out_ch <= 0 || T0 <= 0 || T1 <= 0 || T2 <= 0 || (layout != 0 && layout != 1)) return BTS_ERR_SHAPE;
  if (x == nullptr || y == nullptr || var == nullptr || offsets == nullptr || flips == nullptr || shift == nullptr || scale == nullptr)
    return BTS_ERR_SHAPE;
  if (spatial == nullptr || M == nullptr || phi == nullptr || spacing == nullptr || fill == nullptr) return BTS_ERR_SHAPE;
  for (int n = 0; n < N; ++n) {
    const int* o = offsets + 3 * n;
    if (flips[n] & ~7) return BTS_ERR_SHAPE;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0 || o[0] > S0 - T0 || o[1] > S1 - T1 || o[2] > S2 - T2) return BTS_ERR_SHAPE;
    if (spacing[n] < 1) return BTS_ERR_SHAPE;
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(M[9 * n + k])) return BTS_ERR_SHAPE;
    if (phi[n] != nullptr && (T2 - 1) / spacing[n] + 4 > AUGS_G2MAX) return BTS_ERR_SHAPE;
  }
  const long per_x = (long)T0 * T1 * T2 * C, per_y = (long)T0 * T1 * T2 * out_ch;
  for (int n0 = 0; n0 < N; n0 += AUGS_BATCH_MAX) {
    AugSpatialBatch p;
    p.n = N - n0 < AUGS_BATCH_MAX ? N - n0 : AUGS_BATCH_MAX;
    p.xo = xo + n0 * per_x; p.yo = yo + n0 * per_y;
    p.S0 = S0; p.S1 = S1; p.S2 = S2; p.C = C; p.T0 = T0; p.T1 = T1; p.T2 = T2; p.out_ch = out_ch; p.layout = layout;
    const long planes = (long)p.n * T0;
    long chunks = (2048 + planes - 1) / planes;
    if (chunks > T1) chunks = T1;
    p.rows = (int)((T1 + chunks - 1) / chunks);
    p.chunks = (T1 + p.rows - 1) / p.rows;
    for (int i = 0; i < AUGS_BATCH_MAX; ++i) {
      AugSpatialEntry& e = p.e[i];
      const int n = n0 + (i < p.n ? i : 0);        // (unused entries repeat the first: never read)
      e.x = x[n]; e.y = y[n]; e.var = var[n]; e.phi = phi[n];
      e.o0 = offsets[3 * n]; e.o1 = offsets[3 * n + 1]; e.o2 = offsets[3 * n + 2]; e.flip = flips[n];
      e.spatial = spatial[n] != 0; e.spacing = spacing[n];
      e.G1 = (T1 - 1) / spacing[n] + 4; e.G2 = (T2 - 1) / spacing[n] + 4;
      // a voxel's channels in accesses of 4 or 2 floats where C and the alignment of the volume (and of a channels-last output) allow
      e.xvec = 1;
      for (int v = 4; v > 1; v >>= 1)
        if (C % v == 0 && aug_aligned(e.x, v) && (layout == 1 || aug_aligned(p.xo, v))) { e.xvec = v; break; }
      e.pad = 0; e.pad2 = 0.f;
      for (int k = 0; k < 9; ++k) e.M[k] = M[9 * n + k];
      for (int c = 0; c < AUG_MAXC; ++c) {
        e.shift[c] = c < C ? shift[(long)n * C + c] : 0.f; e.scale[c] = c < C ? scale[(long)n * C + c] : 1.f;
        e.fill[c] = c < C ? fill[(long)n * C + c] : 0.f;
      }
    }
    long blocks = planes * p.chunks;
    if (blocks > 4096) blocks = 4096;
    (void)hipGetLastError(); hipLaunchKernelGGL(augment_spatial_batch_kernel, dim3((int)blocks), dim3(256), 0, stream, p);
    BTS_LAUNCH_CHECK();
  }
  return BTS_OK;
}
