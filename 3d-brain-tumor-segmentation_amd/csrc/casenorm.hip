// Per-case normalisation over the voxels inside a mask, with optional percentile clipping.
// Input: a window (T0,T1,T2,C) of a dense fp32 volume, C innermost, 1 <= C <= 16, addressed in place as prepro.hip does (origin, element
// strides st0 / st1, voxel stride C); an optional fp32 mask window (T0,T1,T2), non-zero = inside; without one a voxel is inside when any
// of its channels is > 0.  Per channel c, over the n voxels inside:
//   lo_c, hi_c  the p_lo / p_hi percentile with linear interpolation, s[k] + f (s[min(k+1,n-1)] - s[k]), h = (n-1) p / 100, k = floor(h),
//               f = h - k, in fp64 (-inf / +inf without clipping)
//   v           clamp(double(x), lo_c, hi_c)
//   mean_c      sum v / n;  std_c = sqrt(sum (v - mean_c)^2 / n), two passes
//   out         float((v - mean_c) / std_c) inside, +0.0 outside; +0.0 everywhere in a channel with std_c == 0 or when n == 0
// Kernels, all on the caller's stream, no host round trip (the ranks come from n on the device):
//   cn_init    zeroes the histograms
//   cn_hist    x 4: one digit of the order-preserving 32-bit key per pass, most significant first; per channel up to four order
//              statistics (k and k+1 of both percentiles) ride in the same pass.  LDS histograms per workgroup, four channels per
//              workgroup (16 KB), merged with 32-bit integer atomics; statistics whose prefixes agree share one histogram
//   cn_pick    x 4: one workgroup finds each statistic's digit; the first derives n and the ranks, the last writes lo / hi
//   cn_sums    x 2: fp64 sums of v, then of (v - mean)^2; a thread owns whole voxels, one partial per workgroup
//   cn_final   x 2: fixed-order sum of the partials -> mean, then std
//   cn_apply   16-byte loads and stores where both addresses allow, float by float elsewhere; labels >= 4 -> 3 ride along
// Integer sums commute and the fp64 sums run in a fixed order: two runs give the same bits.
#include <math.h>
#include "common.h"
#include "bts_internal.h"

#pragma clang fp contract(off)   // the contract is separate fp64 operations, each rounded once

#define CN_MAXC 16
#define CN_BLOCKS 1024       // grid cap of the voxel-owning kernels: 4 workgroups per CU
#define CN_CG 4              // channels per histogram workgroup
#define CN_NQ 4              // order statistics per channel: k_lo, k_lo + 1, k_hi, k_hi + 1
#define CN_BINS 256
#define CN_PASSES 4
#define CN_ROWS 8            // (i0,i1) rows per workgroup visit of the apply pass
#define CN_APPLY_BLOCKS (1L << 20)
// workspace: CN_HDR bytes of state, CN_PASSES x C x CN_NQ x CN_BINS 32-bit counts, CN_BLOCKS x (C + 1) fp64 partials
#define CN_HDR 2048
#define ST_N 0               // 32-bit words of the state
#define ST_PRE 64            // [c * CN_NQ + q]: the key digits found so far
#define ST_REM 128           // [c * CN_NQ + q]: the rank that remains inside them
#define ST_FRAC 128          // in doubles: f of p_lo, f of p_hi

// floats order as these keys: the sign bit set for non-negatives, every bit flipped for negatives (-0.0 sorts just below +0.0)
__device__ __forceinline__ unsigned cn_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cn_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
// numpy's maximum then minimum: the left operand where the comparison holds or it is a NaN
__device__ __forceinline__ double cn_clamp(float x, double lo, double hi) {
  const double d = (double)x;
  const double a = (d >= lo || d != d) ? d : lo;
  return (a <= hi || a != a) ? a : hi;
}

struct CnWin {
  const float* x;
  const float* mask;
  long st0, st1, mst0, mst1;
  unsigned T1, T2, nvox;
  int C;
};

__global__ __launch_bounds__(256) void cn_init_kernel(unsigned* __restrict__ hist, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) hist[i] = 0u;
}

// CT = C where a voxel is one aligned load (C in {1,2,4}), 0 = any C with scalar loads.  -> inside; v[0..NG) = the channels c0.. of the group
template <int CT>
__device__ __forceinline__ bool cn_load_group(const CnWin& w, unsigned i, int c0, int nc, float (&g)[CN_CG]) {
  const unsigned i2 = i % w.T2, row = i / w.T2, i1 = row % w.T1, i0 = row / w.T1;
  if (w.mask != nullptr && w.mask[i0 * w.mst0 + i1 * w.mst1 + i2] == 0.f) return false;
  const float* p = w.x + i0 * w.st0 + i1 * w.st1 + (long)i2 * w.C;
  bool any = w.mask != nullptr;
  if constexpr (CT == 4) { const f32x4 t = *reinterpret_cast<const f32x4*>(p); g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w; }
  else if constexpr (CT == 2) { const float2 t = *reinterpret_cast<const float2*>(p); g[0] = t.x; g[1] = t.y; g[2] = 0.f; g[3] = 0.f; }
  else if constexpr (CT == 1) { g[0] = *p; g[1] = g[2] = g[3] = 0.f; }
  else {
    if (!any)
      for (int c = 0; c < w.C; ++c) any |= p[c] > 0.f;
    if (!any) return false;
#pragma unroll
    for (int k = 0; k < CN_CG; ++k) g[k] = k < nc ? p[c0 + k] : 0.f;
    return true;
  }
  if (!any) {
#pragma unroll
    for (int k = 0; k < CN_CG; ++k) any |= g[k] > 0.f;   // the channels past C hold 0
  }
  return any;
}

template <int CT>
__global__ __launch_bounds__(256) void cn_hist_kernel(CnWin w, const unsigned* __restrict__ state, unsigned* __restrict__ hist, int shift) {
  __shared__ unsigned lh[CN_CG * CN_NQ * CN_BINS];
  __shared__ unsigned spre[CN_CG * CN_NQ];
  __shared__ int suse[CN_CG * CN_NQ];
  const int c0 = blockIdx.y * CN_CG;
  const int nc = w.C - c0 < CN_CG ? w.C - c0 : CN_CG;
  for (int i = threadIdx.x; i < CN_CG * CN_NQ * CN_BINS; i += 256) lh[i] = 0u;
  if (threadIdx.x < CN_CG * CN_NQ) {
    const int k = threadIdx.x / CN_NQ, q = threadIdx.x % CN_NQ;
    unsigned pre = 0u;
    int use = 0;
    if (k < nc) {
      if (shift == 24) use = q == 0;                       // no digit is known yet: one histogram serves every statistic
      else {
        pre = state[ST_PRE + (c0 + k) * CN_NQ + q] >> (shift + 8);
        use = 1;
        for (int r = 0; r < q; ++r)
          if ((state[ST_PRE + (c0 + k) * CN_NQ + r] >> (shift + 8)) == pre) use = 0;   // the first statistic with these digits counts
      }
    }
    spre[threadIdx.x] = pre;
    suse[threadIdx.x] = use;
  }
  __syncthreads();
  unsigned pre[CN_CG][CN_NQ];
  bool use[CN_CG][CN_NQ];
#pragma unroll
  for (int k = 0; k < CN_CG; ++k)
#pragma unroll
    for (int q = 0; q < CN_NQ; ++q) { pre[k][q] = spre[k * CN_NQ + q]; use[k][q] = suse[k * CN_NQ + q] != 0; }
  for (unsigned long i = (unsigned long)blockIdx.x * 256 + threadIdx.x; i < w.nvox; i += (unsigned long)gridDim.x * 256) {
    float g[CN_CG];
    if (!cn_load_group<CT>(w, (unsigned)i, c0, nc, g)) continue;
#pragma unroll
    for (int k = 0; k < CN_CG; ++k) {
      if (k < nc) {
        const unsigned key = cn_key(g[k]);
        const unsigned digit = (key >> shift) & (CN_BINS - 1);
        const unsigned hi = shift == 24 ? 0u : key >> (shift + 8);
#pragma unroll
        for (int q = 0; q < CN_NQ; ++q)
          if (use[k][q] && hi == pre[k][q]) atomicAdd(&lh[(k * CN_NQ + q) * CN_BINS + digit], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nc * CN_NQ * CN_BINS; i += 256)
    if (lh[i]) atomicAdd(&hist[(long)c0 * CN_NQ * CN_BINS + i], lh[i]);
}

// One workgroup, one wave per statistic (c, q), four statistics per round.  The wave reads the histogram of the first statistic of its
// channel that shares its digits so far, four bins per lane; a wave prefix sum finds the lane, and that lane the bin, whose running
// count first passes the rank, and keeps the rank inside that bin.  The first pass has no digits: the bins add up to n, from which the
// ranks follow; the last pass turns the keys back into floats and interpolates.
__global__ __launch_bounds__(256) void cn_pick_kernel(unsigned* __restrict__ state, const unsigned* __restrict__ hist, int C, int shift,
                                                      double p_lo, double p_hi, double* __restrict__ stats) {
  __shared__ unsigned opre[CN_MAXC * CN_NQ];
  __shared__ float sval[CN_MAXC * CN_NQ];
  const bool first = shift == 24, last = shift == 0;
  double* frac = reinterpret_cast<double*>(state) + ST_FRAC;
  if (threadIdx.x < CN_MAXC * CN_NQ) opre[threadIdx.x] = (first || (int)threadIdx.x >= C * CN_NQ) ? 0u : state[ST_PRE + threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s0 = 0; s0 < C * CN_NQ; s0 += 4) {             // C * CN_NQ is a multiple of 4: every wave has a statistic in every round
    const int idx = s0 + wave, q = idx % CN_NQ;
    int rep = 0;
    if (!first) {
      rep = q;
      for (int r = q - 1; r >= 0; --r)
        if ((opre[idx - q + r] >> (shift + 8)) == (opre[idx] >> (shift + 8))) rep = r;
    }
    const unsigned* row = hist + (long)(idx - q + rep) * CN_BINS + lane * 4;
    const unsigned h0 = row[0], h1 = row[1], h2 = row[2], h3 = row[3];
    const unsigned mine = h0 + h1 + h2 + h3;
    unsigned inc = mine;                                  // inclusive prefix sum over the lanes: integers, exact
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
      if (lane >= o) inc += t;
    }
    const unsigned n = (unsigned)__shfl((int)inc, 63, 64);
    unsigned rem;
    if (first) {
      const double p = q < 2 ? p_lo : p_hi;
      const double h = n ? (double)(n - 1u) * p / 100.0 : 0.0;
      const double k = floor(h);
      unsigned rank = (unsigned)k;
      if ((q & 1) && n && rank + 1u < n) rank += 1u;
      rem = rank;
      if (lane == 0 && idx == 0) { state[ST_N] = n; stats[0] = (double)n; frac[0] = h - k; }
      if (lane == 0 && idx == 2) frac[1] = h - k;
    } else {
      rem = state[ST_REM + idx];
    }
    const unsigned exc = inc - mine;
    const bool here = rem >= exc && rem < inc;            // at most one lane; none when the rank is not below the count (n == 0)
    const bool found = __ballot(here) != 0ull;
    if (here) {
      unsigned before = exc, d = 0u;
      if (rem >= before + h0) { before += h0; d = 1u;
        if (rem >= before + h1) { before += h1; d = 2u;
          if (rem >= before + h2) { before += h2; d = 3u; } } }
      const unsigned prefix = opre[idx] | ((unsigned)(lane * 4 + d) << shift);
      state[ST_PRE + idx] = prefix;
      state[ST_REM + idx] = rem - before;
      if (last) sval[idx] = cn_unkey(prefix);
    }
    if (!found && lane == 0) {
      state[ST_PRE + idx] = opre[idx];
      state[ST_REM + idx] = 0u;
      if (last) sval[idx] = cn_unkey(opre[idx]);
    }
  }
  __syncthreads();
  if (last && (int)threadIdx.x < C) {
    const int c = threadIdx.x;
    const bool none = state[ST_N] == 0u;                  // written by the first pass's launch
    const double a0 = (double)sval[c * CN_NQ], a1 = (double)sval[c * CN_NQ + 1];
    const double b0 = (double)sval[c * CN_NQ + 2], b1 = (double)sval[c * CN_NQ + 3];
    stats[1 + 4 * c + 2] = none ? 0.0 : a0 + frac[0] * (a1 - a0);
    stats[1 + 4 * c + 3] = none ? 0.0 : b0 + frac[1] * (b1 - b0);
  }
}

// ---- sums ------------------------------------------------------------------------------------------------------------------------
// second == 0: part[b][c] = sum v, part[b][C] = voxels inside;  second != 0: part[b][c] = sum (v - mean_c)^2.
template <int CT>
__global__ __launch_bounds__(256) void cn_sums_kernel(CnWin w, const double* __restrict__ stats, int clip, int second, double* __restrict__ part) {
  __shared__ double sh[4];
  __shared__ double sm[CN_MAXC], slo[CN_MAXC], shi[CN_MAXC];
  constexpr int NC = CT ? CT : CN_MAXC;
  const int C = w.C;
  if ((int)threadIdx.x < C) {
    sm[threadIdx.x] = second ? stats[1 + 4 * threadIdx.x] : 0.0;
    slo[threadIdx.x] = clip ? stats[1 + 4 * threadIdx.x + 2] : -INFINITY;
    shi[threadIdx.x] = clip ? stats[1 + 4 * threadIdx.x + 3] : INFINITY;
  }
  __syncthreads();
  double s[NC];
  int cnt = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 0.0;
  for (unsigned long i = (unsigned long)blockIdx.x * 256 + threadIdx.x; i < w.nvox; i += (unsigned long)gridDim.x * 256) {
    const unsigned iv = (unsigned)i;
    const unsigned i2 = iv % w.T2, row = iv / w.T2, i1 = row % w.T1, i0 = row / w.T1;
    if (w.mask != nullptr && w.mask[i0 * w.mst0 + i1 * w.mst1 + i2] == 0.f) continue;
    const float* p = w.x + i0 * w.st0 + i1 * w.st1 + (long)i2 * C;
    float v[NC];
    if constexpr (CT == 4) { const f32x4 t = *reinterpret_cast<const f32x4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else if constexpr (CT == 2) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; }
    else {
#pragma unroll
      for (int c = 0; c < NC; ++c) v[c] = (c < C) ? p[c] : 0.f;
    }
    bool any = w.mask != nullptr;
    if (!any) {
#pragma unroll
      for (int c = 0; c < NC; ++c) any |= v[c] > 0.f;
    }
    if (!any) continue;
    ++cnt;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < C) {
        const double d = cn_clamp(v[c], slo[c], shi[c]);
        if (second) { const double e = d - sm[c]; s[c] += e * e; }
        else s[c] += d;
      }
    }
  }
  const long base = (long)blockIdx.x * (C + 1);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < C) {
      const double a = block_sum_f64(s[c], sh);
      if (threadIdx.x == 0) part[base + c] = a;
    }
  }
  const double n = block_sum_f64((double)cnt, sh);      // < 2^31 per thread, exact
  if (threadIdx.x == 0) part[base + C] = n;
}

// one wave per channel: lane l adds partials l, l+64, ... in order, then the fixed-order wave sum
__global__ __launch_bounds__(64) void cn_final_kernel(const double* __restrict__ part, int nblocks, int C, int clip, int second,
                                                      double* __restrict__ stats) {
  const int c = blockIdx.x;
  double t = 0.0, n = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) t += part[(long)b * (C + 1) + c];
  t = wave_sum_f64(t);
  if (clip || second) n = stats[0];                     // the first pick's, or the first finalize's: an earlier launch
  else {
    for (int b = threadIdx.x; b < nblocks; b += 64) n += part[(long)b * (C + 1) + C];
    n = wave_sum_f64(n);
  }
  if (threadIdx.x != 0) return;
  if (!second) {
    if (!clip && c == 0) stats[0] = n;
    stats[1 + 4 * c] = n > 0.0 ? t / n : 0.0;
  } else {
    stats[1 + 4 * c + 1] = n > 0.0 ? sqrt(t / n) : 0.0;
    if (!clip) {
      stats[1 + 4 * c + 2] = n > 0.0 ? -INFINITY : 0.0;
      stats[1 + 4 * c + 3] = n > 0.0 ? INFINITY : 0.0;
    }
    if (n == 0.0) stats[1 + 4 * c] = 0.0;
  }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------
// An item is four consecutive floats of one row, as in crop_norm_kernel.  Whether a float's voxel is inside comes from the mask row or,
// without a mask, from all channels of that voxel: out of the item itself where C divides 4 and the item is whole, re-read elsewhere.
__device__ __forceinline__ float cn_label(float v) { return v >= 4.f ? 3.f : v; }

__global__ __launch_bounds__(256) void cn_apply_kernel(CnWin w, const float* __restrict__ y, long yst0, long yst1, int T0,
                                                       const double* __restrict__ stats, float* __restrict__ xo, float* __restrict__ yo) {
  __shared__ double sm[CN_MAXC], ss[CN_MAXC], slo[CN_MAXC], shi[CN_MAXC];
  __shared__ int szero[CN_MAXC];
  const int C = w.C, T1 = (int)w.T1, T2 = (int)w.T2;
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    const double sd = stats[1 + 4 * c + 1];
    sm[c] = stats[1 + 4 * c]; ss[c] = sd; slo[c] = stats[1 + 4 * c + 2]; shi[c] = stats[1 + 4 * c + 3];
    szero[c] = (stats[0] == 0.0 || sd == 0.0) ? 1 : 0;
  }
  __syncthreads();
  const long rows = (long)T0 * T1;
  const long nbatch = (rows + CN_ROWS - 1) / CN_ROWS;
  const int L = T2 * C, Q = (L + 3) / 4, Qy = (T2 + 3) / 4;
  const bool whole = (4 % C) == 0;                       // C in {1,2,4}: an aligned item holds whole voxels
  for (long bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
    const long row0 = bt * CN_ROWS;
    const int nrow = (int)(rows - row0 < CN_ROWS ? rows - row0 : CN_ROWS);
    for (int i = threadIdx.x; i < nrow * Q; i += 256) {
      const int r = i / Q, e0 = (i - r * Q) * 4;
      const long row = row0 + r;
      const long i0 = row / T1, i1 = row % T1;
      const float* prow = w.x + i0 * w.st0 + i1 * w.st1;
      const float* mrow = w.mask ? w.mask + i0 * w.mst0 + i1 * w.mst1 : nullptr;
      const float* p = prow + e0;
      float* o = xo + row * L + e0;
      const int n = L - e0 < 4 ? L - e0 : 4;
      const bool vec = n == 4 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(o)) & 15) == 0;
      float t[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f};
      if (vec) { const f32x4 q = *reinterpret_cast<const f32x4*>(p); t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w; }
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < n) t[k] = p[k];
      }
      const bool own = mrow == nullptr && whole && n == 4;   // the item's own floats decide
      const bool a0 = t[0] > 0.f, a1 = t[1] > 0.f, a2 = t[2] > 0.f, a3 = t[3] > 0.f;
      const bool h0 = a0 || a1, h1 = a2 || a3, hh = h0 || h1;
      const bool pin[4] = {C == 1 ? a0 : (C == 2 ? h0 : hh), C == 1 ? a1 : (C == 2 ? h0 : hh),
                           C == 1 ? a2 : (C == 2 ? h1 : hh), C == 1 ? a3 : (C == 2 ? h1 : hh)};
      int c = e0 % C, vox = e0 / C, seen = -1;
      bool in = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          if (own) in = pin[k];
          else if (vox != seen) {
            seen = vox;
            if (mrow) in = mrow[vox] != 0.f;
            else {
              in = false;
              for (int j = 0; j < C; ++j) in |= prow[(long)vox * C + j] > 0.f;
            }
          }
          u[k] = (in && !szero[c]) ? (float)((cn_clamp(t[k], slo[c], shi[c]) - sm[c]) / ss[c]) : 0.f;
          if (++c == C) { c = 0; ++vox; }
        }
      }
      if (vec) { f32x4 q; q.x = u[0]; q.y = u[1]; q.z = u[2]; q.w = u[3]; *reinterpret_cast<f32x4*>(o) = q; }
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < n) o[k] = u[k];
      }
    }
    if (y == nullptr) continue;
    for (int i = threadIdx.x; i < nrow * Qy; i += 256) {
      const int r = i / Qy, e0 = (i - r * Qy) * 4;
      const long row = row0 + r;
      const float* p = y + (row / T1) * yst0 + (row % T1) * yst1 + e0;
      float* o = yo + row * T2 + e0;
      if (e0 + 4 <= T2 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        f32x4 v;
        v.x = cn_label(q.x); v.y = cn_label(q.y); v.z = cn_label(q.z); v.w = cn_label(q.w);
        *reinterpret_cast<f32x4*>(o) = v;
      } else {
        const int n = T2 - e0 < 4 ? T2 - e0 : 4;
        for (int k = 0; k < n; ++k) o[k] = cn_label(p[k]);
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
extern "C" int bts_case_norm_blocks(void) { return CN_BLOCKS; }

extern "C" long bts_case_norm_workspace(int C) {
  if (C <= 0 || C > CN_MAXC) return -1;
  return (long)CN_HDR + (long)CN_PASSES * C * CN_NQ * CN_BINS * (long)sizeof(unsigned) + (long)CN_BLOCKS * (C + 1) * (long)sizeof(double);
}

static bool cn_window_ok(long st0, long st1, int T1, int T2, int ld) { return st1 >= (long)T2 * ld && st0 >= (long)T1 * st1; }

template <int CT>
static void cn_launch_hist(const CnWin& w, int blocks, int groups, const unsigned* state, unsigned* hist, int shift, hipStream_t stream) {
  hipLaunchKernelGGL(cn_hist_kernel<CT>, dim3(blocks, groups), dim3(256), 0, stream, w, state, hist, shift);
}
template <int CT>
static void cn_launch_sums(const CnWin& w, int blocks, const double* stats, int clip, int second, double* part, hipStream_t stream) {
  hipLaunchKernelGGL(cn_sums_kernel<CT>, dim3(blocks), dim3(256), 0, stream, w, stats, clip, second, part);
}

extern "C" int bts_case_norm(const float* xwin, long st0, long st1, const float* mask_or_null, long mst0, long mst1,
                             const float* ywin_or_null, long yst0, long yst1, int T0, int T1, int T2, int C, int clip, double p_lo,
                             double p_hi, float* xo, float* yo, double* stats, void* workspace, long workspace_bytes,
                             hipStream_t stream) {
  if (C <= 0 || C > CN_MAXC || T0 <= 0 || T1 <= 0 || T2 <= 0) return BTS_ERR_SHAPE;
  if (!cn_window_ok(st0, st1, T1, T2, C)) return BTS_ERR_SHAPE;
  if (mask_or_null != nullptr && !cn_window_ok(mst0, mst1, T1, T2, 1)) return BTS_ERR_SHAPE;
  if (ywin_or_null != nullptr && (!cn_window_ok(yst0, yst1, T1, T2, 1) || yo == nullptr)) return BTS_ERR_SHAPE;
  if ((long)T0 * T1 > 0x7fffffffL || (long)T0 * T1 * T2 > 0x7fffffffL) return BTS_ERR_SHAPE;
  if ((long)CN_ROWS * ((long)T2 * C + 3) > 0x7fffffffL) return BTS_ERR_SHAPE;       // the apply pass indexes a row batch with an int
  if (clip && !(p_lo >= 0.0 && p_hi <= 100.0 && p_lo <= p_hi)) return BTS_ERR_SHAPE;  // a NaN fails every comparison
  if (xwin == nullptr || xo == nullptr || stats == nullptr) return BTS_ERR_SHAPE;
  if (workspace == nullptr || workspace_bytes < bts_case_norm_workspace(C)) return BTS_ERR_WORKSPACE;
  CnWin w;
  w.x = xwin; w.mask = mask_or_null;
  w.st0 = st0; w.st1 = st1; w.mst0 = mst0; w.mst1 = mst1;
  w.T1 = (unsigned)T1; w.T2 = (unsigned)T2; w.nvox = (unsigned)((long)T0 * T1 * T2);
  w.C = C;
  const long want = ((long)w.nvox + 255) / 256;
  const int blocks = (int)(want < CN_BLOCKS ? want : CN_BLOCKS);
  unsigned* state = reinterpret_cast<unsigned*>(workspace);
  unsigned* hist = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(workspace) + CN_HDR);
  const long per_pass = (long)C * CN_NQ * CN_BINS;
  double* part = reinterpret_cast<double*>(hist + CN_PASSES * per_pass);
  // a voxel is one aligned load where the window origin and both strides are multiples of C floats of C * 4 bytes
  const bool vec = (C == 4 || C == 2) && reinterpret_cast<uintptr_t>(xwin) % (C * 4) == 0 && st0 % C == 0 && st1 % C == 0;
  const int ct = (vec || C == 1) ? C : 0;
  (void)hipGetLastError();
  if (clip) {
    const int total = (int)(CN_PASSES * per_pass);
    hipLaunchKernelGGL(cn_init_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, hist, total);
    BTS_LAUNCH_CHECK();
    const int groups = (C + CN_CG - 1) / CN_CG;
    for (int p = 0; p < CN_PASSES; ++p) {
      const int shift = 8 * (CN_PASSES - 1 - p);
      unsigned* h = hist + p * per_pass;
      if (ct == 4) cn_launch_hist<4>(w, blocks, groups, state, h, shift, stream);
      else if (ct == 2) cn_launch_hist<2>(w, blocks, groups, state, h, shift, stream);
      else if (ct == 1) cn_launch_hist<1>(w, blocks, groups, state, h, shift, stream);
      else cn_launch_hist<0>(w, blocks, groups, state, h, shift, stream);
      BTS_LAUNCH_CHECK();
      hipLaunchKernelGGL(cn_pick_kernel, dim3(1), dim3(256), 0, stream, state, h, C, shift, p_lo, p_hi, stats);
      BTS_LAUNCH_CHECK();
    }
  }
  for (int second = 0; second < 2; ++second) {
    if (ct == 4) cn_launch_sums<4>(w, blocks, stats, clip, second, part, stream);
    else if (ct == 2) cn_launch_sums<2>(w, blocks, stats, clip, second, part, stream);
    else if (ct == 1) cn_launch_sums<1>(w, blocks, stats, clip, second, part, stream);
    else cn_launch_sums<0>(w, blocks, stats, clip, second, part, stream);
    BTS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cn_final_kernel, dim3(C), dim3(64), 0, stream, part, blocks, C, clip, second, stats);
    BTS_LAUNCH_CHECK();
  }
  const long nbatch = ((long)T0 * T1 + CN_ROWS - 1) / CN_ROWS;
  const unsigned ab = (unsigned)(nbatch < CN_APPLY_BLOCKS ? nbatch : CN_APPLY_BLOCKS);
  hipLaunchKernelGGL(cn_apply_kernel, dim3(ab), dim3(256), 0, stream, w, ywin_or_null, yst0, yst1, T0, stats, xo, yo);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
