// The distance side of the per-case score (test.py:266-270): what the 95th-percentile Hausdorff distance of a region needs
// on the device.
//   region_surface  surface voxels (a face neighbour outside the region or outside the volume) of one region of a uint8 label map, and
//                   their number
//   edt3d_sq        exact squared Euclidean distance transform in mm^2 to the nearest feature voxel, float64, three separable passes
//   masked_select   exact order statistics of the selected values of a float64 buffer by radix select, no host round trip
// Dense tensors, W innermost.  Plain HIP C++: vector loads and stores, integer atomics only, no inline assembly.  Every loop count is a
// function of the shape alone, no kernel waits on another workgroup, and every result is the same bits in every run.
#include "common.h"
#include "bts_internal.h"

#include <math.h>

#define SURF_MAXK 8
#define SURF_BLOCKS 2048          // grid cap of the streaming kernels: 8 workgroups per CU
#define EDT_LDS_DOUBLES 8192      // 64 KiB of LDS per workgroup: a whole line tile
#define SEL_MAXRANKS 8
#define SEL_BINS 256              // radix select digit: 8 bits, 8 passes over a 64-bit key
#define SEL_PASSES 8
#define SEL_STATE 32              // 64-bit words of state in front of the histograms: per rank (prefix, remaining rank, valid, unused)
#define SEL_BLOCKS 1024

// ---- region surface -------------------------------------------------------------------------------------------------------------
// An item is four consecutive voxels of the flat volume: one 4-byte load of the labels and one 4-byte store of the flags where both maps
// are 4-byte aligned (VEC), byte by byte otherwise and in the tail.  A voxel of the region is a surface voxel unless all six face
// neighbours exist and belong to the region; the neighbour bytes are only read for voxels of the region that are off the volume's border,
// so every index is inside the volume.  Counts: per thread in a register, per workgroup in LDS, one 64-bit integer atomic per workgroup.
__device__ __forceinline__ unsigned in_region(unsigned lab, unsigned top, unsigned class_mask) {
  return (class_mask >> (lab < top ? lab : top)) & 1u;
}

template <bool VEC>
__global__ __launch_bounds__(256) void region_surface_kernel(const uint8_t* __restrict__ lab, uint8_t* __restrict__ surf,
                                                             unsigned long long* count, int D, int H, int W, long nvox, long nitems,
                                                             unsigned top, unsigned class_mask) {
  __shared__ unsigned long long wg_count;
  if (threadIdx.x == 0) wg_count = 0ull;
  __syncthreads();
  const long HW = (long)H * W;
  unsigned long long mine = 0ull;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < nitems; it += (long)gridDim.x * 256) {
    const long v0 = it * 4;
    const int n = nvox - v0 < 4 ? (int)(nvox - v0) : 4;
    unsigned centre = 0u;
    if (VEC && n == 4) {
      centre = *reinterpret_cast<const unsigned*>(lab + v0);
    } else {
      for (int k = 0; k < n; ++k) centre |= (unsigned)lab[v0 + k] << (8 * k);
    }
    long d = v0 / HW;
    const long r = v0 - d * HW;
    int h = (int)(r / W), w = (int)(r - (long)h * W);
    unsigned flags = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        if (in_region((centre >> (8 * k)) & 255u, top, class_mask)) {
          const long v = v0 + k;
          unsigned all = 0u;
          if (w > 0 && w < W - 1 && h > 0 && h < H - 1 && d > 0 && d < D - 1) {
            all = in_region(lab[v - 1], top, class_mask) & in_region(lab[v + 1], top, class_mask) &
                  in_region(lab[v - W], top, class_mask) & in_region(lab[v + W], top, class_mask) &
                  in_region(lab[v - HW], top, class_mask) & in_region(lab[v + HW], top, class_mask);
          }
          if (!all) {
            flags |= 1u << (8 * k);
            ++mine;
          }
        }
        if (++w == W) {
          w = 0;
          if (++h == H) { h = 0; ++d; }
        }
      }
    }
    if (VEC && n == 4) {
      *reinterpret_cast<unsigned*>(surf + v0) = flags;
    } else {
      for (int k = 0; k < n; ++k) surf[v0 + k] = (uint8_t)((flags >> (8 * k)) & 255u);
    }
  }
  if (mine) atomicAdd(&wg_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && wg_count) atomicAdd(count, wg_count);
}

extern "C" int bts_region_surface(const uint8_t* lab, uint8_t* surf, long* count, int D, int H, int W, int K, int class_mask,
                                  hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || K < 2 || K > SURF_MAXK) return BTS_ERR_SHAPE;
  if (class_mask < 0 || class_mask >= (1 << K)) return BTS_ERR_SHAPE;
  const long nvox = (long)D * H * W;
  const long nitems = (nvox + 3) / 4;
  long blocks = (nitems + 255) / 256;
  blocks = blocks > SURF_BLOCKS ? SURF_BLOCKS : blocks;
  const bool vec = ((reinterpret_cast<uintptr_t>(lab) | reinterpret_cast<uintptr_t>(surf)) & 3) == 0;
  unsigned long long* c = reinterpret_cast<unsigned long long*>(count);
  (void)hipGetLastError();
  if (vec) hipLaunchKernelGGL(region_surface_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, lab, surf, c, D, H, W, nvox, nitems,
                              (unsigned)K - 1u, (unsigned)class_mask);
  else hipLaunchKernelGGL(region_surface_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, lab, surf, c, D, H, W, nvox, nitems,
                          (unsigned)K - 1u, (unsigned)class_mask);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- squared Euclidean distance transform -------------------------------------------------------------------------------------
// Along an axis of spacing s: out[i] = min_j ( g[j] + (s (i - j)) (s (i - j)) ), every product and the sum rounded once (the
// compiler's default contraction rule would fuse the sum with the square into one fma, also through __dmul_rn / __dadd_rn, which are
// plain * and + inlined with that rule attached: the operators are written out under a pragma that forbids it), the minimum over ALL j of the line: fixed work, and a minimum does not depend on the order it
// is taken in.  g is +inf where there is no feature, and +inf + x = +inf, so no value is ever a NaN.  A workgroup stages whole lines in LDS
// before it writes any of them, which is what lets the H and D passes run in place.
__device__ __forceinline__ double edt_line_min(const double* __restrict__ g, int stride, int L, int i, double s) {
#pragma clang fp contract(off)
  double best = INFINITY;
#pragma unroll 4
  for (int j = 0; j < L; ++j) {
    const double t = s * (double)(i - j);
    const double tt = t * t;
    best = fmin(best, g[(long)j * stride] + tt);
  }
  return best;
}

// W pass: a workgroup owns RW whole rows (contiguous in memory), g = 0 on features and +inf elsewhere; lanes run along the row.
__global__ __launch_bounds__(256) void edt_pass_w_kernel(const uint8_t* __restrict__ feat, double* __restrict__ dist2, long rows, int W,
                                                         int RW, double s) {
  extern __shared__ double g[];
  const long row0 = (long)blockIdx.x * RW;
  const int nrow = (int)(rows - row0 < RW ? rows - row0 : RW);
  const int ne = nrow * W;                                        // <= EDT_LDS_DOUBLES
  const uint8_t* f = feat + row0 * W;
  for (int e = threadIdx.x; e < ne; e += 256) g[e] = f[e] ? 0.0 : (double)INFINITY;
  __syncthreads();
  double* o = dist2 + row0 * W;
  for (int e = threadIdx.x; e < ne; e += 256) {
    const int r = e / W, i = e - r * W;
    o[e] = edt_line_min(g + r * W, 1, W, i, s);
  }
}

// H and D passes, in place: the volume is (outer, L, inner) with the pass along L.  A workgroup owns the L x TW tile of TW consecutive
// inner positions (TW = 16 doubles, one 128-byte line, while the tile fits LDS): lanes run along `inner`, so a wave reads and writes
// whole lines, and in LDS 16 consecutive doubles with the other lanes of the wave on the same addresses (a broadcast).
__global__ __launch_bounds__(256) void edt_pass_strided_kernel(double* __restrict__ dist2, int L, long inner, int TW, int tw_shift,
                                                               long tiles, double s) {
  extern __shared__ double g[];
  const long outer = (long)blockIdx.x / tiles;
  const long t0 = ((long)blockIdx.x - outer * tiles) * TW;
  const int tw = (int)(inner - t0 < TW ? inner - t0 : TW);
  double* base = dist2 + outer * L * inner + t0;
  const int ne = L * TW;                                          // <= EDT_LDS_DOUBLES
  for (int e = threadIdx.x; e < ne; e += 256) {
    const int j = e >> tw_shift, c = e & (TW - 1);
    if (c < tw) g[e] = base[(long)j * inner + c];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ne; e += 256) {
    const int i = e >> tw_shift, c = e & (TW - 1);
    if (c < tw) base[(long)i * inner + c] = edt_line_min(g + c, TW, L, i, s);
  }
}

static int edt_strided_pass(double* dist2, long outer, int L, long inner, double s, hipStream_t stream) {
  if (L == 1) return BTS_OK;                                      // g + (s 0)(s 0) = g, bit for bit: nothing to do
  int TW = 16, shift = 4;
  while (TW > 1 && (long)L * TW > EDT_LDS_DOUBLES) { TW >>= 1; --shift; }
  const long tiles = (inner + TW - 1) / TW;
  const long blocks = outer * tiles;
  hipLaunchKernelGGL(edt_pass_strided_kernel, dim3((unsigned)blocks), dim3(256), (size_t)L * TW * sizeof(double), stream, dist2, L, inner,
                     TW, shift, tiles, s);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_edt3d_sq(const uint8_t* feat, double* dist2, int D, int H, int W, double sd, double sh, double sw,
                            hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0) return BTS_ERR_SHAPE;
  if (!(sd > 0.0) || !(sh > 0.0) || !(sw > 0.0) || isinf(sd) || isinf(sh) || isinf(sw)) return BTS_ERR_SHAPE;
  if (D > EDT_LDS_DOUBLES || H > EDT_LDS_DOUBLES || W > EDT_LDS_DOUBLES) return BTS_ERR_SHAPE;     // a line must fit LDS
  const long rows = (long)D * H;
  int RW = 1024 / W;                                              // about a thousand outputs per workgroup
  RW = RW < 1 ? 1 : RW;
  const long wblocks = (rows + RW - 1) / RW;
  // grids: one workgroup per tile, fewer than 2^31 of them
  const long hblocks = (long)D * (((long)W + 15) / 16), dblocks = ((long)H * W + 15) / 16;
  if (wblocks > 0x7fffffffL || hblocks * 16 > 0x7fffffffL || dblocks * 16 > 0x7fffffffL) return BTS_ERR_SHAPE;
  (void)hipGetLastError();
  hipLaunchKernelGGL(edt_pass_w_kernel, dim3((unsigned)wblocks), dim3(256), (size_t)RW * W * sizeof(double), stream, feat, dist2, rows, W,
                     RW, sw);
  BTS_LAUNCH_CHECK();
  int r = edt_strided_pass(dist2, D, H, W, sh, stream);
  if (r != BTS_OK) return r;
  return edt_strided_pass(dist2, 1, D, (long)H * W, sd, stream);
}

// ---- masked select --------------------------------------------------------------------------------------------------------------
// Non-negative doubles order as their 64-bit patterns.  Per pass (most significant digit first) and per requested rank: a histogram of
// the pass's digit over the selected values whose higher digits equal the rank's prefix so far (LDS integer atomics per workgroup,
// merged with global 64-bit integer atomics), then one workgroup picks the digit that holds the rank and the rank that remains inside
// it.  Integer sums commute, so the answer is exact and the same bits in every run.
// work: SEL_STATE 64-bit words of state, then [pass][rank][SEL_BINS] 64-bit counts, all written by select_init_kernel.
struct SelRanks {
  long r[SEL_MAXRANKS];
};

__global__ __launch_bounds__(256) void select_init_kernel(unsigned long long* __restrict__ work, SelRanks ranks, int nranks, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  unsigned long long x = 0ull;
  if (i < SEL_STATE && (i & 3) == 1) {
#pragma unroll
    for (int q = 0; q < SEL_MAXRANKS; ++q)
      if (q == (i >> 2) && q < nranks) x = (unsigned long long)ranks.r[q];
  }
  work[i] = x;
}

// An item is four consecutive elements: one 4-byte load of the mask where it is 4-byte aligned (VEC); a value is only loaded where its
// mask byte is set.
template <bool VEC>
__global__ __launch_bounds__(256) void select_hist_kernel(const unsigned long long* __restrict__ v, const uint8_t* __restrict__ mask,
                                                          long n, long nitems, const unsigned long long* __restrict__ state,
                                                          unsigned long long* __restrict__ hist, int nranks, int shift) {
  __shared__ unsigned int lh[SEL_MAXRANKS * SEL_BINS];
  for (int i = threadIdx.x; i < nranks * SEL_BINS; i += 256) lh[i] = 0u;
  __syncthreads();
  unsigned long long pre[SEL_MAXRANKS];                           // the digits above this pass's, per rank
#pragma unroll
  for (int q = 0; q < SEL_MAXRANKS; ++q) pre[q] = (q < nranks && shift < 56) ? state[q * 4] >> (shift + 8) : 0ull;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < nitems; it += (long)gridDim.x * 256) {
    const long v0 = it * 4;
    const int nn = n - v0 < 4 ? (int)(n - v0) : 4;
    unsigned mw = 0u;
    if (VEC && nn == 4) {
      mw = *reinterpret_cast<const unsigned*>(mask + v0);
    } else {
      for (int k = 0; k < nn; ++k) mw |= (unsigned)mask[v0 + k] << (8 * k);
    }
    if (mw == 0u) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((mw >> (8 * k)) & 255u) {                               // (a set byte lies inside n: the bytes past it were never loaded)
        const unsigned long long key = v[v0 + k];
        const unsigned digit = (unsigned)(key >> shift) & (SEL_BINS - 1);
        const unsigned long long hi = shift < 56 ? key >> (shift + 8) : 0ull;
#pragma unroll
        for (int q = 0; q < SEL_MAXRANKS; ++q)
          if (q < nranks && hi == pre[q]) atomicAdd(&lh[q * SEL_BINS + digit], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nranks * SEL_BINS; i += 256)
    if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

__global__ __launch_bounds__(256) void select_pick_kernel(unsigned long long* __restrict__ state, const unsigned long long* __restrict__ hist,
                                                          int nranks, int shift, int first, int last, double* __restrict__ out) {
  __shared__ unsigned long long c[SEL_MAXRANKS * SEL_BINS];
  for (int i = threadIdx.x; i < nranks * SEL_BINS; i += 256) c[i] = hist[i];
  __syncthreads();
  if ((int)threadIdx.x < nranks) {
    const int q = threadIdx.x;
    const unsigned long long rem = state[q * 4 + 1];
    unsigned long long valid = state[q * 4 + 2];
    unsigned long long cum = 0ull, before = 0ull;
    unsigned digit = 0u;
    bool found = false;
    for (int b = 0; b < SEL_BINS; ++b) {                          // all bins, always: the first bin whose running count passes the rank
      const unsigned long long nc = cum + c[q * SEL_BINS + b];
      if (!found && rem < nc) {
        found = true;
        digit = (unsigned)b;
        before = cum;
      }
      cum = nc;
    }
    if (first) valid = found ? 1ull : 0ull;                       // the rank is below the number of selected values
    const unsigned long long prefix = state[q * 4] | (found ? (unsigned long long)digit << shift : 0ull);
    state[q * 4] = prefix;
    state[q * 4 + 1] = found ? rem - before : 0ull;
    state[q * 4 + 2] = valid;
    if (last) reinterpret_cast<unsigned long long*>(out)[q] = valid ? prefix : 0x7ff8000000000000ull;
  }
}

extern "C" long bts_masked_select_workspace(int nranks) {
  if (nranks < 1 || nranks > SEL_MAXRANKS) return BTS_ERR_SHAPE;
  return (long)(SEL_STATE + (long)SEL_PASSES * nranks * SEL_BINS) * (long)sizeof(unsigned long long);
}

extern "C" int bts_masked_select(const double* v, const uint8_t* mask, long n, const long* ranks, int nranks, double* out, void* work,
                                 hipStream_t stream) {
  if (n < 0 || n > (1L << 40) || nranks < 0 || nranks > SEL_MAXRANKS) return BTS_ERR_SHAPE;
  if (nranks > 0 && ranks == nullptr) return BTS_ERR_SHAPE;
  SelRanks rk;
  for (int q = 0; q < SEL_MAXRANKS; ++q) {
    rk.r[q] = q < nranks ? ranks[q] : 0;
    if (rk.r[q] < 0) return BTS_ERR_SHAPE;
  }
  if (n == 0 || nranks == 0) return BTS_OK;
  unsigned long long* w = static_cast<unsigned long long*>(work);
  const int total = SEL_STATE + SEL_PASSES * nranks * SEL_BINS;
  const long nitems = (n + 3) / 4;
  long blocks = (nitems + 255) / 256;
  blocks = blocks > SEL_BLOCKS ? SEL_BLOCKS : blocks;
  const bool vec = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(v);
  (void)hipGetLastError();
  hipLaunchKernelGGL(select_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, rk, nranks, total);
  BTS_LAUNCH_CHECK();
  for (int p = 0; p < SEL_PASSES; ++p) {
    const int shift = 8 * (SEL_PASSES - 1 - p);
    unsigned long long* hist = w + SEL_STATE + (long)p * nranks * SEL_BINS;
    if (vec) hipLaunchKernelGGL(select_hist_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, keys, mask, n, nitems, w, hist, nranks, shift);
    else hipLaunchKernelGGL(select_hist_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, keys, mask, n, nitems, w, hist, nranks, shift);
    BTS_LAUNCH_CHECK();
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(256), 0, stream, w, hist, nranks, shift, p == 0 ? 1 : 0, p == SEL_PASSES - 1 ? 1 : 0, out);
    BTS_LAUNCH_CHECK();
  }
  return BTS_OK;
}
