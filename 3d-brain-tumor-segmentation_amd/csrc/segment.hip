// The two passes of the reference's test.py main() that no other file covers (test.py:181-270).
//   skull_strip      x * (1 - p) of the skull stage, the crop to the unpadded extent and the padding to the tumour model's resolution,
//                    with the brain mask carried along, in one pass (test.py:244-254)
//   label_confusion  K x K integer counts of (truth, prediction) label pairs, the only device-side work of the per-case score
//                    (test.py:226-232,266-270)
// Dense tensors, C innermost.  Plain HIP C++: vector loads and stores, integer atomics, no inline assembly.
#include "common.h"
#include "bts_internal.h"

#define SEG_ROWS 8           // output (d,h) rows per workgroup
#define SEG_MAXWG (1L << 24) // a launch holds fewer than 2^32 threads: fewer than 2^24 workgroups of 256
#define SEG_BLOCKS 1024      // label_confusion grid cap: 4 workgroups per CU
#define SEG_MAXK 8

// ---- skull strip ---------------------------------------------------------------------------------------------------------------
// An item is four consecutive floats of one OUTPUT row (of xo: Wb*C floats, of mo: Wb).  Rows outside (D,H) and items past W*C (W) are
// zero stores; an item wholly inside moves as one 16-byte load and one 16-byte store where both addresses allow; an item that straddles
// the edge, sits in a short tail or is misaligned goes float by float.  One IEEE fp32 subtract and one fp32 multiply per value
// (__fsub_rn / __fmul_rn: never contracted), the value numpy's float32 expression x * (1 - p) stores.  Row bases are 64-bit.
__device__ __forceinline__ float strip1(float x, float p) { return __fmul_rn(x, __fsub_rn(1.0f, p)); }

// A wave owns whole rows (wave w of the workgroup: rows w and w + 4 of its 8), so the row's (d,h), its padding test and its input row base
// are found once per row, not per item; lanes stride over the row's items.  e0 / C is a shift where C is a power of two.
__global__ __launch_bounds__(256) void skull_strip_kernel(const float* __restrict__ x, const float* __restrict__ p,
                                                          const float* __restrict__ m, float* __restrict__ xo, float* __restrict__ mo,
                                                          int Ha, int Wa, int D, int H, int W, int Db, int Hb, int Wb, int C) {
  const long rows = (long)Db * Hb;
  const long row0 = (long)blockIdx.x * SEG_ROWS;
  const int nrow = (int)(rows - row0 < SEG_ROWS ? rows - row0 : SEG_ROWS);
  const int L = Wb * C, Lin = W * C, Q = (L + 3) / 4, Qm = (Wb + 3) / 4;
  const int lane = threadIdx.x & 63;
  const int cshift = (C & (C - 1)) == 0 ? __builtin_ctz((unsigned)C) : -1;
  for (int r = threadIdx.x >> 6; r < nrow; r += 4) {
    const long row = row0 + r;
    const int d = (int)(row / Hb), h = (int)(row - (long)d * Hb);
    const bool pad_row = d >= D || h >= H;
    const long vin = pad_row ? 0 : ((long)d * Ha + h) * Wa;       // first voxel of the input row; a padding row has none and reads nothing
    float* orow = xo + row * L;
    const float* xrow = x + vin * C;
    const float* pi = p + vin;
    for (int e0 = lane * 4; e0 < Q * 4; e0 += 256) {
      float* o = orow + e0;
      const int n = L - e0 < 4 ? L - e0 : 4;
      const bool oal = n == 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
      if (pad_row || e0 >= Lin) {                                // padding
        if (oal) *reinterpret_cast<f32x4*>(o) = f32x4{0.f, 0.f, 0.f, 0.f};
        else for (int k = 0; k < n; ++k) o[k] = 0.f;
        continue;
      }
      const float* xi = xrow + e0;
      int w = cshift >= 0 ? e0 >> cshift : e0 / C, c = e0 - w * C;
      if (oal && e0 + 4 <= Lin && (reinterpret_cast<uintptr_t>(xi) & 15) == 0) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xi);
        f32x4 v;                                                 // (every pi[w] below has w < W: the item ends inside the row)
        v.x = strip1(t.x, pi[w]); if (++c == C) { c = 0; ++w; }
        v.y = strip1(t.y, pi[w]); if (++c == C) { c = 0; ++w; }
        v.z = strip1(t.z, pi[w]); if (++c == C) { c = 0; ++w; }
        v.w = strip1(t.w, pi[w]);
        *reinterpret_cast<f32x4*>(o) = v;
      } else {
        for (int k = 0; k < n; ++k) {
          o[k] = (e0 + k < Lin) ? strip1(xi[k], pi[w]) : 0.f;
          if (++c == C) { c = 0; ++w; }
        }
      }
    }
    float* omrow = mo + row * Wb;
    const float* mrow = m + vin;
    for (int e0 = lane * 4; e0 < Qm * 4; e0 += 256) {
      float* o = omrow + e0;
      const int n = Wb - e0 < 4 ? Wb - e0 : 4;
      const bool oal = n == 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0;
      if (pad_row || e0 >= W) {
        if (oal) *reinterpret_cast<f32x4*>(o) = f32x4{0.f, 0.f, 0.f, 0.f};
        else for (int k = 0; k < n; ++k) o[k] = 0.f;
        continue;
      }
      const float* mi = mrow + e0;
      if (oal && e0 + 4 <= W && (reinterpret_cast<uintptr_t>(mi) & 15) == 0) {
        *reinterpret_cast<f32x4*>(o) = *reinterpret_cast<const f32x4*>(mi);
      } else {
        for (int k = 0; k < n; ++k) o[k] = (e0 + k < W) ? mi[k] : 0.f;
      }
    }
  }
}

extern "C" int bts_skull_strip(const float* x, const float* p, const float* m, float* xo, float* mo, int Da, int Ha, int Wa, int D,
                               int H, int W, int Db, int Hb, int Wb, int C, hipStream_t stream) {
  if (C < 1) return BTS_ERR_SHAPE;
  if (Da <= 0 || Ha <= 0 || Wa <= 0 || D <= 0 || H <= 0 || W <= 0 || Db <= 0 || Hb <= 0 || Wb <= 0) return BTS_ERR_SHAPE;
  if (D > Da || H > Ha || W > Wa || D > Db || H > Hb || W > Wb) return BTS_ERR_SHAPE;
  if ((long)SEG_ROWS * ((long)Wb * C + 3) > 0x7fffffffL || (long)Wa * C > 0x7fffffffL) return BTS_ERR_SHAPE;   // in-row indices are int
  const long nb = ((long)Db * Hb + SEG_ROWS - 1) / SEG_ROWS;
  if (nb >= SEG_MAXWG) return BTS_ERR_SHAPE;
  (void)hipGetLastError();
  hipLaunchKernelGGL(skull_strip_kernel, dim3((unsigned)nb), dim3(256), 0, stream, x, p, m, xo, mo, Ha, Wa, D, H, W, Db, Hb, Wb, C);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- label confusion -----------------------------------------------------------------------------------------------------------
// A chunk is 16 consecutive voxels: one 16-byte load per map where both maps sit equally far from a 16-byte boundary (VEC; the up to 15
// voxels before the first boundary and after the last whole chunk go one by one), byte loads otherwise.  A lane merges runs of equal
// (t,p) pairs -- label maps are piecewise constant along a row -- and adds each run with one integer atomic to its wave's LDS histogram;
// pair (0,0), nearly all of a scan, is counted in a register.  A workgroup then adds each non-zero bin to the global counts with one
// 64-bit integer atomic.  Integer sums commute: the counts are exact and the same bits in every run, whatever the order.
__device__ __forceinline__ int pair_bin(unsigned t, unsigned p, int K) {
  const unsigned top = (unsigned)K - 1u;
  return (int)((t < top ? t : top) * (unsigned)K + (p < top ? p : top));
}

struct RunCounter {
  int cur, run;
  unsigned long long zero;
  unsigned long long* hist;
  __device__ __forceinline__ void flush() {
    if (run == 0) return;
    if (cur == 0) zero += (unsigned)run;
    else atomicAdd(&hist[cur], (unsigned long long)run);
  }
  __device__ __forceinline__ void add(int bin) {
    if (bin == cur) { ++run; return; }
    flush();
    cur = bin;
    run = 1;
  }
  __device__ __forceinline__ void add_word(unsigned tw, unsigned pw, int K) {
#pragma unroll
    for (int b = 0; b < 4; ++b) add(pair_bin((tw >> (8 * b)) & 255u, (pw >> (8 * b)) & 255u, K));
  }
};

template <bool VEC>
__global__ __launch_bounds__(256) void label_confusion_kernel(const uint8_t* __restrict__ truth, const uint8_t* __restrict__ pred,
                                                              long nvox, long head, long nchunks, int K,
                                                              unsigned long long* counts) {
  __shared__ unsigned long long hist[4][SEG_MAXK * SEG_MAXK];
  for (int i = threadIdx.x; i < 4 * SEG_MAXK * SEG_MAXK; i += 256) (&hist[0][0])[i] = 0ull;
  __syncthreads();
  RunCounter rc;
  rc.cur = -1;
  rc.run = 0;
  rc.zero = 0ull;
  rc.hist = hist[threadIdx.x >> 6];
  for (long ch = (long)blockIdx.x * 256 + threadIdx.x; ch < nchunks; ch += (long)gridDim.x * 256) {
    const long v0 = head + ch * 16;
    if constexpr (VEC) {
      const uint4 t = *reinterpret_cast<const uint4*>(truth + v0);
      const uint4 q = *reinterpret_cast<const uint4*>(pred + v0);
      rc.add_word(t.x, q.x, K);
      rc.add_word(t.y, q.y, K);
      rc.add_word(t.z, q.z, K);
      rc.add_word(t.w, q.w, K);
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) rc.add(pair_bin(truth[v0 + k], pred[v0 + k], K));
    }
  }
  if (blockIdx.x == 0) {                    // the voxels outside the chunks: fewer than 32, one per lane
    const long tail0 = head + nchunks * 16;
    const long ntail = nvox - tail0;
    const long t = threadIdx.x;
    if (t < head) rc.add(pair_bin(truth[t], pred[t], K));
    else if (t >= 16 && t - 16 < ntail) rc.add(pair_bin(truth[tail0 + t - 16], pred[tail0 + t - 16], K));
  }
  rc.flush();
  if (rc.zero) atomicAdd(&rc.hist[0], rc.zero);
  __syncthreads();
  if (threadIdx.x < K * K) {
    const unsigned long long s = hist[0][threadIdx.x] + hist[1][threadIdx.x] + hist[2][threadIdx.x] + hist[3][threadIdx.x];
    if (s) atomicAdd(&counts[threadIdx.x], s);
  }
}

extern "C" int bts_label_confusion(const uint8_t* truth, const uint8_t* pred, long nvox, int K, long* counts, hipStream_t stream) {
  if (K < 2 || K > SEG_MAXK || nvox < 0) return BTS_ERR_SHAPE;
  if (nvox == 0) return BTS_OK;
  const uintptr_t a = reinterpret_cast<uintptr_t>(truth), b = reinterpret_cast<uintptr_t>(pred);
  const bool vec = ((a ^ b) & 15) == 0;
  long head = vec ? (long)((16 - (a & 15)) & 15) : 0;
  if (head > nvox) head = nvox;
  const long nchunks = (nvox - head) / 16;
  long blocks = (nchunks + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > SEG_BLOCKS ? SEG_BLOCKS : blocks);
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  (void)hipGetLastError();
  if (vec) hipLaunchKernelGGL(label_confusion_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, truth, pred, nvox, head, nchunks, K, c);
  else hipLaunchKernelGGL(label_confusion_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, truth, pred, nvox, head, nchunks, K, c);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
