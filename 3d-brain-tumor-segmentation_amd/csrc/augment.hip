// GPU-side training augmentation (reference train.py:14-49, a tf.data map on the host).
// Per example: per-channel intensity shift/scale driven by the volume's per-channel standard deviation, a random
// crop_size window of the (x,y) pair, per-axis flips, and one-hot labels without the background channel.
// The random draws are arguments (the TF stream cannot be reproduced); given the draws the arithmetic is the
// reference's: x <- (x + shift*sqrt(var)) * scale in fp32, var = population variance over the whole volume.
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
