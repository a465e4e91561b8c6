// The nested BraTS regions as training targets and as the decoded prediction: channel order (WT, TC, ET) = labels {1,2,4}, {1,4}, {4}
// (infer.BRATS_REGIONS).  Three single streaming passes, all for C == 3 only:
//   bts_region_targets    one-hot(label) minus background, as the augment kernels leave it  ->  region targets, in place
//   bts_region_dice_sums  hard Dice counts per region (p > 0.5 against t > 0.5) and the decoded label map of a training step
//   bts_region_finish     the counterpart of bts_tta_finish: prob * bmask and the region -> label decode of a segmented volume
// A channels-last voxel is 12 bytes, so a lane takes FOUR voxels = 48 bytes as three 16-byte accesses (the label rows of augment.hip are
// stored the same way); a group that is not whole (the last N*V mod 4 voxels) or a base that is not 16-byte aligned (a view into a larger
// buffer) goes voxel by voxel.  No inline assembly; no floating-point atomics except the per-workgroup adds of integer-valued doubles.
#include "common.h"
#include "bts_internal.h"

#define REGION_C 3
#define REGION_BLOCKS 2048   // memory-bound grid cap (8 workgroups of 256 per CU), grid-stride beyond it

__device__ __forceinline__ void region_ld4(const float* p, float* r) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
}
__device__ __forceinline__ void region_st4(float* p, const float* r) { *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]); }
__device__ __forceinline__ bool region_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// (l1, l2, l3) -> (wt, tc, et) = ((l1 + l2) + l3, l1 + l3, l3)
__device__ __forceinline__ void region_encode(float& a, float& b, float& c) {
  const float wt = (a + b) + c, tc = a + c;
  a = wt; b = tc;
}
// the overwrite rule of the BraTS conversions (ET over TC over WT), `on` = the three comparisons already taken
__device__ __forceinline__ int region_label(bool wt, bool tc, bool et, int et_value) { return et ? et_value : (tc ? 1 : (wt ? 2 : 0)); }

// ---------------------------------------------------------------------------------------------
// targets.  layout 0: y (NV, 3), groups of four voxels over the whole batch; layout 1: y (N, 3, V), groups of four voxels along the planes
// of one example (its three planes are V floats apart), a group is vectorised when the example's three plane starts are 16-byte aligned.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void region_targets_last_kernel(float* __restrict__ y, long NV) {
  const long groups = (NV + 3) / 4;
  const bool vec = region_aligned16(y);
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    float* p = y + g * 12;
    if (vec && 4 * g + 4 <= NV) {
      float r[12];
      region_ld4(p, r); region_ld4(p + 4, r + 4); region_ld4(p + 8, r + 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) region_encode(r[3 * e], r[3 * e + 1], r[3 * e + 2]);
      region_st4(p, r); region_st4(p + 4, r + 4); region_st4(p + 8, r + 8);
    } else {
      const int n = (int)((NV - 4 * g < 4) ? NV - 4 * g : 4);
      for (int e = 0; e < n; ++e) {
        float a = p[3 * e], b = p[3 * e + 1], c = p[3 * e + 2];
        region_encode(a, b, c);
        p[3 * e] = a; p[3 * e + 1] = b;
      }
    }
  }
}
__global__ __launch_bounds__(256) void region_targets_first_kernel(float* __restrict__ y, int N, long V) {
  const long per = (V + 3) / 4, groups = (long)N * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < groups; i += (long)gridDim.x * blockDim.x) {
    const long n = i / per, g = i - n * per;
    float* p0 = y + n * 3 * V + 4 * g;
    float* p1 = p0 + V;
    float* p2 = p1 + V;
    if (4 * g + 4 <= V && region_aligned16(p0) && region_aligned16(p1) && region_aligned16(p2)) {
      float a[4], b[4], c[4];
      region_ld4(p0, a); region_ld4(p1, b); region_ld4(p2, c);
#pragma unroll
      for (int e = 0; e < 4; ++e) region_encode(a[e], b[e], c[e]);
      region_st4(p0, a); region_st4(p1, b);
    } else {
      const int m = (int)((V - 4 * g < 4) ? V - 4 * g : 4);
      for (int e = 0; e < m; ++e) {
        float a = p0[e], b = p1[e], c = p2[e];
        region_encode(a, b, c);
        p0[e] = a; p1[e] = b;
      }
    }
  }
}
extern "C" int bts_region_targets(float* y, int N, long V, int C, int channels_first, hipStream_t stream) {
  if (C != REGION_C) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || V <= 0 || y == nullptr) return BTS_ERR_SHAPE;
  const long NV = (long)N * V;
  const long groups = channels_first ? (long)N * ((V + 3) / 4) : (NV + 3) / 4;
  long blocks = (groups + 255) / 256;
  if (blocks > REGION_BLOCKS) blocks = REGION_BLOCKS;
  (void)hipGetLastError();
  if (channels_first) hipLaunchKernelGGL(region_targets_first_kernel, dim3((int)blocks), dim3(256), 0, stream, y, N, V);
  else hipLaunchKernelGGL(region_targets_last_kernel, dim3((int)blocks), dim3(256), 0, stream, y, NV);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Dice counts.  table[3r + {0,1,2}] = (I_r, P_r, T_r) as doubles (zeroed here), the layout bts_dice_metric_value reduces with one cell per
// channel.  Every lane counts in nine integer registers, the counts are summed over the wave and the workgroup, and a workgroup adds
// one value per entry: integers below 2^53, so the double sums are exact and the table is bit-identical whatever the order of the adds.
// labels[v] = 3 | 1 | 2 | 0 by the overwrite rule with p > 0.5 (the coding of DiceCoefficient.last_labels: 3 is ET).
// ---------------------------------------------------------------------------------------------
__global__ void region_zero_kernel(double* p, int n) {
  if (threadIdx.x < n) p[threadIdx.x] = 0.0;
}
__device__ __forceinline__ int region_count(const float* t, const float* p, unsigned* cnt) {
  const bool pw = p[0] > 0.5f, pt = p[1] > 0.5f, pe = p[2] > 0.5f;
  const bool tw = t[0] > 0.5f, tt = t[1] > 0.5f, te = t[2] > 0.5f;
  cnt[0] += (pw && tw) ? 1u : 0u; cnt[1] += pw ? 1u : 0u; cnt[2] += tw ? 1u : 0u;
  cnt[3] += (pt && tt) ? 1u : 0u; cnt[4] += pt ? 1u : 0u; cnt[5] += tt ? 1u : 0u;
  cnt[6] += (pe && te) ? 1u : 0u; cnt[7] += pe ? 1u : 0u; cnt[8] += te ? 1u : 0u;
  return region_label(pw, pt, pe, 3);
}
__global__ __launch_bounds__(256) void region_dice_kernel(const float* __restrict__ ytrue, const float* __restrict__ ypred,
                                                          uint8_t* __restrict__ labels, double* table, long NV, int ldt, int ldp) {
  __shared__ double sh[4][9];
  unsigned cnt[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) cnt[k] = 0u;
  const long groups = (NV + 3) / 4;
  // four voxels per lane where both tensors are dense and aligned (labels: one 4-byte store); otherwise a voxel at a time
  const bool vec = ldt == 3 && ldp == 3 && region_aligned16(ytrue) && region_aligned16(ypred) &&
                   (labels == nullptr || (reinterpret_cast<uintptr_t>(labels) & 3) == 0);
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    if (vec && 4 * g + 4 <= NV) {
      float t[12], p[12];
      region_ld4(ytrue + g * 12, t); region_ld4(ytrue + g * 12 + 4, t + 4); region_ld4(ytrue + g * 12 + 8, t + 8);
      region_ld4(ypred + g * 12, p); region_ld4(ypred + g * 12 + 4, p + 4); region_ld4(ypred + g * 12 + 8, p + 8);
      int lbl[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) lbl[e] = region_count(t + 3 * e, p + 3 * e, cnt);
      if (labels) *reinterpret_cast<uchar4*>(labels + 4 * g) = make_uchar4((uint8_t)lbl[0], (uint8_t)lbl[1], (uint8_t)lbl[2], (uint8_t)lbl[3]);
    } else {
      const int n = (int)((NV - 4 * g < 4) ? NV - 4 * g : 4);
      for (int e = 0; e < n; ++e) {
        const long v = 4 * g + e;
        const float t[3] = {ytrue[v * ldt], ytrue[v * ldt + 1], ytrue[v * ldt + 2]};
        const float p[3] = {ypred[v * ldp], ypred[v * ldp + 1], ypred[v * ldp + 2]};
        const int lbl = region_count(t, p, cnt);
        if (labels) labels[v] = (uint8_t)lbl;
      }
    }
  }
  // (all 64 lanes are back together here: wave_sum_f64 needs the whole wave)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double s = wave_sum_f64((double)cnt[k]);
    if (lane == 0) sh[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const double s = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
    if (s != 0.0) atomicAdd(table + threadIdx.x, s);
  }
}
extern "C" int bts_region_dice_sums(const float* y_true, const float* y_pred, uint8_t* labels, double* table, long NV, int C, int ldt,
                                    int ldp, hipStream_t stream) {
  if (C != REGION_C) return BTS_ERR_UNSUPPORTED;
  if (NV <= 0 || ldt < C || ldp < C) return BTS_ERR_SHAPE;
  (void)hipGetLastError(); hipLaunchKernelGGL(region_zero_kernel, dim3(1), dim3(64), 0, stream, table, 9);
  BTS_LAUNCH_CHECK();
  long blocks = ((NV + 3) / 4 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  (void)hipGetLastError(); hipLaunchKernelGGL(region_dice_kernel, dim3((int)blocks), dim3(256), 0, stream, y_true, y_pred, labels, table, NV, ldt,
                     ldp);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// finish.  y = prob * bmask; label = 4 if et >= threshold, else 1 if tc >= threshold, else 2 if wt >= threshold, else 0, of the MASKED
// probabilities, and 0 wherever bmask == 0 (>= as in tta_finish_kernel, which zeroes best < threshold).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int region_finish_voxel(float* pv, float m, float threshold) {
  pv[0] *= m; pv[1] *= m; pv[2] *= m;
  const int lbl = region_label(pv[0] >= threshold, pv[1] >= threshold, pv[2] >= threshold, 4);
  return m == 0.f ? 0 : lbl;
}
__global__ __launch_bounds__(256) void region_finish_kernel(const float* __restrict__ prob, const float* __restrict__ bmask, float* y,
                                                            uint8_t* labels, long nvox, float threshold) {
  const long groups = (nvox + 3) / 4;
  const bool vec = region_aligned16(prob) && region_aligned16(bmask) && (y == nullptr || region_aligned16(y)) &&
                   (labels == nullptr || (reinterpret_cast<uintptr_t>(labels) & 3) == 0);
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    if (vec && 4 * g + 4 <= nvox) {
      float p[12], m[4];
      region_ld4(prob + g * 12, p); region_ld4(prob + g * 12 + 4, p + 4); region_ld4(prob + g * 12 + 8, p + 8);
      region_ld4(bmask + g * 4, m);
      int lbl[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) lbl[e] = region_finish_voxel(p + 3 * e, m[e], threshold);
      if (y) { region_st4(y + g * 12, p); region_st4(y + g * 12 + 4, p + 4); region_st4(y + g * 12 + 8, p + 8); }
      if (labels) *reinterpret_cast<uchar4*>(labels + 4 * g) = make_uchar4((uint8_t)lbl[0], (uint8_t)lbl[1], (uint8_t)lbl[2], (uint8_t)lbl[3]);
    } else {
      const int n = (int)((nvox - 4 * g < 4) ? nvox - 4 * g : 4);
      for (int e = 0; e < n; ++e) {
        const long v = 4 * g + e;
        float p[3] = {prob[v * 3], prob[v * 3 + 1], prob[v * 3 + 2]};
        const int lbl = region_finish_voxel(p, bmask[v], threshold);
        if (y) { y[v * 3] = p[0]; y[v * 3 + 1] = p[1]; y[v * 3 + 2] = p[2]; }
        if (labels) labels[v] = (uint8_t)lbl;
      }
    }
  }
}
extern "C" int bts_region_finish(const float* prob, const float* bmask, float* y, uint8_t* labels, long nvox, int C, float threshold,
                                 hipStream_t stream) {
  if (C != REGION_C) return BTS_ERR_UNSUPPORTED;
  if (nvox <= 0) return BTS_ERR_SHAPE;
  long blocks = ((nvox + 3) / 4 + 255) / 256;
  if (blocks > REGION_BLOCKS) blocks = REGION_BLOCKS;
  (void)hipGetLastError(); hipLaunchKernelGGL(region_finish_kernel, dim3((int)blocks), dim3(256), 0, stream, prob, bmask, y, labels, nvox,
                     threshold);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
