// Ensembles of tumour models and their voxel-wise uncertainty maps (infer.StageEnsemble, infer.uncertainty_scores).
// Three single streaming passes:
//   bts_ensemble_update        Welford's recurrence over one member's mean probabilities: running mean and sum of squared deviations
//   bts_uncertainty_finish     running mean (entropy) or spread (deviation) -> one uint8 level 0..100 per voxel and channel, 0 off the mask
//   bts_uncertainty_confusion  counts per channel, level and (truth, prediction) pair: the table uncertainty-filtered Dice is reduced from
// The float passes take FOUR consecutive floats per lane as one 16-byte access per tensor where every base is 16-byte aligned and the
// group is whole; a group that is not (the last n mod 4 floats) or a base that is not (a view into a larger buffer) goes float by float.
// No inline assembly; no floating-point atomics (the counts are integers).
#include "common.h"
#include "bts_internal.h"

#define ENS_BLOCKS 2048      // memory-bound grid cap (8 workgroups of 256 per CU), grid-stride beyond it
#define UNC_LEVELS 101       // levels 0..100
#define UNC_MAXC 4           // channels of a map: the three regions, or up to four classes
#define UNC_MAXK 8           // classes of a label map, as bts_label_confusion

__device__ __forceinline__ bool ens_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ void ens_ld4(const float* p, float* r) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
}
__device__ __forceinline__ void ens_st4(float* p, const float* r) { *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]); }

// ---------------------------------------------------------------------------------------------
// update.  d = p - mean; mean += d / k; m2 += d * (p - mean), every operation rounded once on its own (contraction into an fma is
// switched off in ens_step; the division is the IEEE one), so the result is the float32 numpy recurrence bit for bit.  FIRST (k == 1):
// mean = p, m2 = 0, the accumulators are not read.  WITH_M2 false: only the mean is kept.  Bytes per float: 8 (first) | 12 (mean only) | 20.
// ---------------------------------------------------------------------------------------------
template <bool WITH_M2>
__device__ __forceinline__ void ens_step(float p, float& mean, float& m2, float kf) {
#pragma clang fp contract(off)      // plain operators under the pragma: __fmul_rn inside __fadd_rn still becomes one fma after inlining
  const float d = p - mean;
  mean = mean + __fdiv_rn(d, kf);
  if (WITH_M2) {
    const float t = d * (p - mean);
    m2 = m2 + t;
  }
}

template <bool FIRST, bool WITH_M2>
__global__ __launch_bounds__(256) void ensemble_update_kernel(const float* __restrict__ p, float* __restrict__ mean, float* __restrict__ m2,
                                                              long n, float kf) {
  const long groups = (n + 3) / 4;
  const bool vec = ens_aligned16(p) && ens_aligned16(mean) && (!WITH_M2 || ens_aligned16(m2));
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long i0 = 4 * g;
    if (vec && i0 + 4 <= n) {
      float a[4], m[4], s[4] = {0.f, 0.f, 0.f, 0.f};
      ens_ld4(p + i0, a);
      if (FIRST) {
        ens_st4(mean + i0, a);
        if (WITH_M2) ens_st4(m2 + i0, s);
      } else {
        ens_ld4(mean + i0, m);
        if (WITH_M2) ens_ld4(m2 + i0, s);
#pragma unroll
        for (int e = 0; e < 4; ++e) ens_step<WITH_M2>(a[e], m[e], s[e], kf);
        ens_st4(mean + i0, m);
        if (WITH_M2) ens_st4(m2 + i0, s);
      }
    } else {
      const int cnt = (int)((n - i0 < 4) ? n - i0 : 4);
      for (int e = 0; e < cnt; ++e) {
        const long i = i0 + e;
        if (FIRST) {
          mean[i] = p[i];
          if (WITH_M2) m2[i] = 0.f;
        } else {
          float m = mean[i], s = WITH_M2 ? m2[i] : 0.f;
          ens_step<WITH_M2>(p[i], m, s, kf);
          mean[i] = m;
          if (WITH_M2) m2[i] = s;
        }
      }
    }
  }
}

extern "C" int bts_ensemble_update(const float* p, float* mean, float* m2, long n, int k, hipStream_t stream) {
  if (n <= 0 || k < 1 || p == nullptr || mean == nullptr) return BTS_ERR_SHAPE;
  if (p == mean || p == m2 || mean == m2) return BTS_ERR_UNSUPPORTED;
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > ENS_BLOCKS) blocks = ENS_BLOCKS;
  const dim3 grid((unsigned)blocks), block(256);
  const float kf = (float)k;
  (void)hipGetLastError();
  if (k == 1) {
    if (m2) hipLaunchKernelGGL((ensemble_update_kernel<true, true>), grid, block, 0, stream, p, mean, m2, n, kf);
    else hipLaunchKernelGGL((ensemble_update_kernel<true, false>), grid, block, 0, stream, p, mean, m2, n, kf);
  } else {
    if (m2) hipLaunchKernelGGL((ensemble_update_kernel<false, true>), grid, block, 0, stream, p, mean, m2, n, kf);
    else hipLaunchKernelGGL((ensemble_update_kernel<false, false>), grid, block, 0, stream, p, mean, m2, n, kf);
  }
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// finish.  One level per voxel and channel, channels last, 0 where bmask == 0.
//   mode 0  p = clamp(mean, 0, 1), h = -(p log2 p + (1 - p) log2(1 - p)), 0 at p in {0, 1}; level = min(100, floor(100 h + 0.5))
//   mode 1  level = min(100, floor(200 sqrt(max(spread, 0) scale) + 0.5))
// A lane takes four consecutive levels: one 16-byte load, one 4-byte store; the voxel of the first is found by one division (by a
// constant for C = 1, 3, 4) and the others by counting on.  Bytes per level: 4 + 4 / C + 1.  (Sixteen levels per lane with one 16-byte
// store were measured and are slower, 22.8 against 20.9 us at 160x192x160x3: the pass is bound by its arithmetic per level, not its stores.)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned unc_round(float t) {
  const float r = floorf(t + 0.5f);
  return (unsigned)(r < 100.f ? (r > 0.f ? r : 0.f) : 100.f);           // (a NaN compares false twice: level 100)
}
__device__ __forceinline__ unsigned unc_entropy(float v) {
  const float p = fminf(fmaxf(v, 0.f), 1.f), q = 1.f - p;
  if (!(p > 0.f && q > 0.f)) return v != v ? 100u : 0u;                 // p in {0, 1}: no uncertainty; a NaN mean: all of it
  const float h = -(p * log2f(p) + q * log2f(q));
  return unc_round(100.f * h);
}
__device__ __forceinline__ unsigned unc_std(float s, float scale) { return unc_round(200.f * sqrtf(fmaxf(s, 0.f) * scale)); }

template <int CT, int MODE>
__global__ __launch_bounds__(256) void uncertainty_finish_kernel(const float* __restrict__ src, const float* __restrict__ bmask,
                                                                 uint8_t* __restrict__ unc, long n, int Crt, float scale) {
  const int C = CT > 0 ? CT : Crt;
  const long groups = (n + 3) / 4;
  const bool vec = ens_aligned16(src) && (reinterpret_cast<uintptr_t>(unc) & 3) == 0;
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long i0 = 4 * g;
    long v = i0 / C;
    int c = (int)(i0 - v * C);
    const int cnt = (int)((n - i0 < 4) ? n - i0 : 4);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    const bool whole = vec && cnt == 4;
    if (whole) ens_ld4(src + i0, a);
    else for (int e = 0; e < cnt; ++e) a[e] = src[i0 + e];
    unsigned lv[4] = {0u, 0u, 0u, 0u};
    float m = bmask[v];                                                  // (i0 < n: v is a voxel of the volume)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const unsigned l = MODE == 0 ? unc_entropy(a[e]) : unc_std(a[e], scale);
        lv[e] = m == 0.f ? 0u : l;
        if (++c == C) {
          c = 0;
          ++v;
          if (e + 1 < cnt) m = bmask[v];                                 // (the next level exists, and so does its voxel)
        }
      }
    }
    if (whole) *reinterpret_cast<unsigned*>(unc + i0) = lv[0] | (lv[1] << 8) | (lv[2] << 16) | (lv[3] << 24);
    else for (int e = 0; e < cnt; ++e) unc[i0 + e] = (uint8_t)lv[e];
  }
}

template <int CT>
static void unc_finish_launch(int mode, dim3 grid, hipStream_t stream, const float* src, const float* bmask, uint8_t* unc, long n, int C,
                              float scale) {
  if (mode == 0) hipLaunchKernelGGL((uncertainty_finish_kernel<CT, 0>), grid, dim3(256), 0, stream, src, bmask, unc, n, C, scale);
  else hipLaunchKernelGGL((uncertainty_finish_kernel<CT, 1>), grid, dim3(256), 0, stream, src, bmask, unc, n, C, scale);
}

extern "C" int bts_uncertainty_finish(const float* mean, const float* spread, const float* bmask, uint8_t* unc, long nvox, int C, int mode,
                                      float scale, hipStream_t stream) {
  if (mode != 0 && mode != 1) return BTS_ERR_UNSUPPORTED;
  if (nvox <= 0 || C < 1 || C > 1024 || bmask == nullptr || unc == nullptr) return BTS_ERR_SHAPE;
  const float* src = mode == 0 ? mean : spread;
  if (src == nullptr || (mode == 1 && !(scale >= 0.f))) return BTS_ERR_SHAPE;
  const long n = nvox * C;
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > ENS_BLOCKS) blocks = ENS_BLOCKS;
  const dim3 grid((unsigned)blocks);
  (void)hipGetLastError();
  switch (C) {
    case 1: unc_finish_launch<1>(mode, grid, stream, src, bmask, unc, n, C, scale); break;
    case 3: unc_finish_launch<3>(mode, grid, stream, src, bmask, unc, n, C, scale); break;
    case 4: unc_finish_launch<4>(mode, grid, stream, src, bmask, unc, n, C, scale); break;
    default: unc_finish_launch<0>(mode, grid, stream, src, bmask, unc, n, C, scale); break;
  }
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// confusion.  table[c][level][2 t + pr] += 1 per voxel with mask != 0 and channel c, t / pr = is min(label, K-1) of truth / prediction a
// class of class_masks[c]; a level above 100 counts as 100.  label_confusion_kernel's pattern: a chunk is 16 consecutive voxels (16-byte
// loads where every map is 16-byte aligned and the chunk is whole, byte loads otherwise); every wave counts in its own LDS table of
// C * 101 * 4 cells, 32-bit (fewer than 2^31 voxels per call, so no cell can wrap; four waves' tables of four channels are 25.9 kB), except
// cell (level 0, t 0, pr 0) of each channel, nearly all of a scan, which a lane counts in a register; a workgroup then adds each
// non-zero cell to the global table with one 64-bit integer atomic.  Integer sums commute: exact, and the same bits in every run.
// ---------------------------------------------------------------------------------------------
struct UncMasks { unsigned m[UNC_MAXC]; };

__device__ __forceinline__ unsigned unc_byte(const uint4& q, int k) {
  const unsigned w = k < 8 ? (k < 4 ? q.x : q.y) : (k < 12 ? q.z : q.w);
  return (w >> (8 * (k & 3))) & 255u;
}

template <int C>
__device__ __forceinline__ void unc_count(unsigned t, unsigned p, const unsigned* u, const UncMasks& cm, unsigned top, unsigned* hist,
                                          unsigned* zero) {
  t = t < top ? t : top;
  p = p < top ? p : top;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const unsigned lvl = u[c] < 100u ? u[c] : 100u;
    const unsigned cell = (lvl << 2) | (((cm.m[c] >> t) & 1u) << 1) | ((cm.m[c] >> p) & 1u);
    if (cell == 0u) ++zero[c];
    else atomicAdd(&hist[c * (UNC_LEVELS * 4) + cell], 1u);
  }
}

template <int C>
__global__ __launch_bounds__(256) void uncertainty_confusion_kernel(const uint8_t* __restrict__ truth, const uint8_t* __restrict__ pred,
                                                                    const uint8_t* __restrict__ unc, const uint8_t* __restrict__ mask,
                                                                    long nvox, int K, UncMasks cm, unsigned long long* table) {
  constexpr int CELLS = C * UNC_LEVELS * 4;
  __shared__ unsigned hist[4][CELLS];
  for (int i = threadIdx.x; i < 4 * CELLS; i += 256) (&hist[0][0])[i] = 0u;
  __syncthreads();
  unsigned* mine = hist[threadIdx.x >> 6];
  unsigned zero[C];
#pragma unroll
  for (int c = 0; c < C; ++c) zero[c] = 0u;
  const unsigned top = (unsigned)K - 1u;
  const long nchunks = (nvox + 15) / 16;
  const bool vec = ens_aligned16(truth) && ens_aligned16(pred) && ens_aligned16(unc) && (mask == nullptr || ens_aligned16(mask));
  for (long ch = (long)blockIdx.x * 256 + threadIdx.x; ch < nchunks; ch += (long)gridDim.x * 256) {
    const long v0 = ch * 16;
    if (vec && v0 + 16 <= nvox) {
      const uint4 t = *reinterpret_cast<const uint4*>(truth + v0);
      const uint4 q = *reinterpret_cast<const uint4*>(pred + v0);
      uint4 m = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
      if (mask) m = *reinterpret_cast<const uint4*>(mask + v0);
      uint4 uq[C];                                                       // 16 voxels x C levels: C whole 16-byte loads
#pragma unroll
      for (int j = 0; j < C; ++j) uq[j] = *reinterpret_cast<const uint4*>(unc + v0 * C + 16 * j);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (unc_byte(m, k) == 0u) continue;
        unsigned u[C];
#pragma unroll
        for (int c = 0; c < C; ++c) u[c] = unc_byte(uq[(k * C + c) >> 4], (k * C + c) & 15);
        unc_count<C>(unc_byte(t, k), unc_byte(q, k), u, cm, top, mine, zero);
      }
    } else {
      const int cnt = (int)((nvox - v0 < 16) ? nvox - v0 : 16);
      for (int k = 0; k < cnt; ++k) {
        const long v = v0 + k;
        if (mask && mask[v] == 0) continue;
        unsigned u[C];
#pragma unroll
        for (int c = 0; c < C; ++c) u[c] = unc[v * C + c];
        unc_count<C>(truth[v], pred[v], u, cm, top, mine, zero);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (zero[c]) atomicAdd(&mine[c * (UNC_LEVELS * 4)], zero[c]);
  __syncthreads();
  for (int i = threadIdx.x; i < CELLS; i += 256) {
    const unsigned long long s = (unsigned long long)hist[0][i] + hist[1][i] + hist[2][i] + hist[3][i];
    if (s) atomicAdd(&table[i], s);
  }
}

extern "C" int bts_uncertainty_confusion(const uint8_t* truth, const uint8_t* pred, const uint8_t* unc, const uint8_t* mask, long nvox,
                                         int C, int K, const unsigned* class_masks, unsigned long long* table, hipStream_t stream) {
  if (C < 1 || C > UNC_MAXC) return BTS_ERR_UNSUPPORTED;
  if (K < 2 || K > UNC_MAXK || nvox < 0 || nvox >= 0x7fffffffL || class_masks == nullptr) return BTS_ERR_SHAPE;
  UncMasks cm;
  for (int c = 0; c < UNC_MAXC; ++c) {
    cm.m[c] = c < C ? class_masks[c] : 0u;
    if (cm.m[c] >> K) return BTS_ERR_SHAPE;
  }
  if (nvox == 0) return BTS_OK;
  if (truth == nullptr || pred == nullptr || unc == nullptr || table == nullptr) return BTS_ERR_SHAPE;
  long blocks = ((nvox + 15) / 16 + 255) / 256;
  if (blocks > ENS_BLOCKS) blocks = ENS_BLOCKS;
  const dim3 grid((unsigned)blocks), block(256);
  (void)hipGetLastError();
  switch (C) {
    case 1: hipLaunchKernelGGL((uncertainty_confusion_kernel<1>), grid, block, 0, stream, truth, pred, unc, mask, nvox, K, cm, table); break;
    case 2: hipLaunchKernelGGL((uncertainty_confusion_kernel<2>), grid, block, 0, stream, truth, pred, unc, mask, nvox, K, cm, table); break;
    case 3: hipLaunchKernelGGL((uncertainty_confusion_kernel<3>), grid, block, 0, stream, truth, pred, unc, mask, nvox, K, cm, table); break;
    default: hipLaunchKernelGGL((uncertainty_confusion_kernel<4>), grid, block, 0, stream, truth, pred, unc, mask, nvox, K, cm, table); break;
  }
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
