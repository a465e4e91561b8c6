// Device-side spline resampling of a scan to the 1 mm^3 grid and back (reference test.py:15-72: Interpolator calls
// scipy.ndimage.zoom(order=3, mode='reflect'), builds the brain mask and, after the model, zooms the prediction back).
// Tensors are dense fp32 (D,H,W,C), C innermost, 1 <= C <= 8; every channel is resampled on its own.  All offsets are 64-bit.
//
//   bts_spline_prefilter3d  cubic B-spline coefficients: per axis, line *= 6, causal recursion c_i += z c_{i-1} from the exact
//                           half-sample-symmetric ('reflect') initial value, anti-causal c_i = z (c_{i+1} - c_i), z = sqrt(3) - 2.
//                           D and H lines are coalesced across (w,c) and run in global memory; W lines (stride C) run on tiles of
//                           whole rows staged in LDS, so global traffic along W is whole cache lines, read once and written once.
//   bts_zoom3d              one thread per output voxel, all C channels in registers: 1 / 8 / 64 taps (order 0 / 1 / 3) with reflect
//                           index mapping, the brain mask from the same registers, zero fill of the padding region.
#include "common.h"
#include "bts_internal.h"
#include "resample_taps.h"

#define RS_POLE (-0.26794919243112270647f)  // sqrt(3) - 2
// terms of the initial-value sum: all of them for n <= 32; beyond that the dropped ones weigh |z|^32 = 5e-19 of the line
#define RS_HORIZON 32
#define RS_LDS_BYTES 32768

// one line of n samples, `stride` floats apart: s -> d (s == d allowed; every element is read before it is written)
__device__ __forceinline__ void rs_filter_line(const float* s, float* d, long stride, int n, float gain, float zn) {
  const float z = RS_POLE;
  const int K = n < RS_HORIZON ? n : RS_HORIZON;
  float zi = 1.f, head = 0.f, tail = 0.f;
  for (int i = 0; i < K; ++i) {
    head += zi * s[(long)i * stride];
    tail += zi * s[(long)(n - 1 - i) * stride];
    zi *= z;
  }
  float prev = 6.f * s[0] + gain * (6.f * (head + zn * tail));  // c0 + z/(1 - z^2n) * sum z^i (c_i + z^n c_{n-1-i})
  d[0] = prev;
  for (int i = 1; i < n; i += 8) {  // loads of a chunk are issued together; the recursion then runs from registers
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (i + k < n) ? s[(long)(i + k) * stride] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i + k < n) { prev = 6.f * v[k] + z * prev; d[(long)(i + k) * stride] = prev; }
  }
  float cur = prev * (z / (z - 1.f));
  d[(long)(n - 1) * stride] = cur;
  for (int i = n - 2; i >= 0; i -= 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (i - k >= 0) ? d[(long)(i - k) * stride] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i - k >= 0) { cur = z * (cur - v[k]); d[(long)(i - k) * stride] = cur; }
  }
}

// lines of an axis of extent n whose samples are `inner` floats apart: line L = (outer, j), base = outer * n * inner + j.
// Consecutive threads take consecutive j, so every access of a wave is one contiguous run when inner >= 64.
__global__ __launch_bounds__(256) void rs_prefilter_lines_kernel(const float* src, float* dst, long nlines, long inner, int n,
                                                                 float gain, float zn) {
  for (long L = blockIdx.x * 256L + threadIdx.x; L < nlines; L += (long)gridDim.x * 256L) {
    const long outer = L / inner, j = L - outer * inner;
    const long base = outer * (long)n * inner + j;
    rs_filter_line(src + base, dst + base, inner, n, gain, zn);
  }
}

// W axis: a block stages R whole rows (R * W * C contiguous floats) in LDS with pitch `pitch`, R * C threads each filter one
// (row, channel) line there, then the rows go back.  pitch % 32 == C % 32, so the lanes of a wave touch consecutive banks.
__global__ __launch_bounds__(256) void rs_prefilter_rows_kernel(const float* src, float* dst, long nrows, int W, int C, int R,
                                                                int pitch, float gain, float zn) {
  extern __shared__ float rs_tile[];
  const int WC = W * C;
  for (long row0 = (long)blockIdx.x * R; row0 < nrows; row0 += (long)gridDim.x * R) {
    const int rows = (int)((nrows - row0 < R) ? nrows - row0 : R);
    for (int r = 0; r < rows; ++r)
      for (int q = threadIdx.x; q < WC; q += 256) rs_tile[r * pitch + q] = src[(row0 + r) * WC + q];
    __syncthreads();
    if ((int)threadIdx.x < rows * C) {
      const int r = threadIdx.x / C, c = threadIdx.x - r * C;
      float* line = rs_tile + r * pitch + c;
      rs_filter_line(line, line, C, W, gain, zn);
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r)
      for (int q = threadIdx.x; q < WC; q += 256) dst[(row0 + r) * WC + q] = rs_tile[r * pitch + q];
    __syncthreads();
  }
}

static void rs_line_constants(int n, float* gain, float* zn) {
  const double z = sqrt(3.0) - 2.0;
  *zn = (float)pow(z, (double)n);
  *gain = (float)(z / (1.0 - pow(z, 2.0 * (double)n)));
}

static int rs_launch_lines(const float* src, float* dst, long nlines, long inner, int n, hipStream_t stream) {
  float gain, zn;
  rs_line_constants(n, &gain, &zn);
  long blocks = (nlines + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  (void)hipGetLastError(); hipLaunchKernelGGL(rs_prefilter_lines_kernel, dim3((int)blocks), dim3(256), 0, stream, src, dst, nlines, inner, n,
                     gain, zn);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_spline_prefilter3d(const float* src, float* dst, int D, int H, int W, int C, hipStream_t stream) {
  if (D < 4 || H < 4 || W < 4 || C < 1 || C > RS_MAXC) return BTS_ERR_SHAPE;
  const long HWC = (long)H * W * C, WC = (long)W * C;
  int r = rs_launch_lines(src, dst, HWC, HWC, D, stream);                 // along D: lines (h,w,c), samples H*W*C apart
  if (r != BTS_OK) return r;
  r = rs_launch_lines(dst, dst, (long)D * WC, WC, H, stream);             // along H: lines (d; w,c), samples W*C apart
  if (r != BTS_OK) return r;
  const long nrows = (long)D * H;
  const int pitch = (int)WC + (int)(((C - WC % 32) + 32) % 32);
  int R = 256 / C;
  if ((long)R * pitch * 4 > RS_LDS_BYTES) R = (int)(RS_LDS_BYTES / ((long)pitch * 4));
  if (R < 1) return rs_launch_lines(dst, dst, nrows * C, C, W, stream);   // a row that does not fit in LDS: strided lines
  float gain, zn;
  rs_line_constants(W, &gain, &zn);
  long blocks = (nrows + R - 1) / R;
  if (blocks > 65536) blocks = 65536;
  (void)hipGetLastError(); hipLaunchKernelGGL(rs_prefilter_rows_kernel, dim3((int)blocks), dim3(256), (size_t)R * pitch * 4, stream, dst, dst, nrows,
                     W, C, R, pitch, gain, zn);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

struct ZoomParams {
  const float* coef;
  float* dst;
  float* bmask;
  const float* mean;
  const float* stdv;
  int Din, Hin, Win, Dout, Hout, Wout, Dpad, Hpad, Wpad;
  double sd, sh, sw;  // (n - 1) / (nout - 1) per axis, as zoom() forms it
};

// NT taps per axis: 1 = order 0 (nearest, floor(c + 0.5)), 2 = order 1, 4 = order 3 on prefiltered coefficients.
// Order 1 sums its 8 taps as zoom() does, ((v * wd) * wh) * ww in row-major tap order; order 3 sums separably, W innermost.
template <int C, int NT>
__global__ __launch_bounds__(256) void rs_zoom_kernel(const ZoomParams p) {
  const long total = (long)p.Dpad * p.Hpad * p.Wpad;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    long v = i;
    const int w = (int)(v % p.Wpad); v /= p.Wpad;
    const int h = (int)(v % p.Hpad);
    const int d = (int)(v / p.Hpad);
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    if (d < p.Dout && h < p.Hout && w < p.Wout) {
      int id[NT], ih[NT], iw[NT];
      float wd[NT], wh[NT], ww[NT];
      rs_taps<NT>(d, p.sd, p.Din, id, wd);
      rs_taps<NT>(h, p.sh, p.Hin, ih, wh);
      rs_taps<NT>(w, p.sw, p.Win, iw, ww);
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        float ah[C];
#pragma unroll
        for (int c = 0; c < C; ++c) ah[c] = 0.f;
#pragma unroll
        for (int b = 0; b < NT; ++b) {
          const float* row = p.coef + ((long)id[a] * p.Hin + ih[b]) * p.Win * C;
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
    if (p.bmask) {  // test.py:53-54: mask = max over channels > 0, from the raw resampled values
      float mx = acc[0];
#pragma unroll
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, acc[c]);
      p.bmask[i] = mx > 0.f ? 1.f : 0.f;
    }
    if (p.mean) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = (acc[c] - p.mean[c]) / p.stdv[c];
    }
    rs_store<C>(p.dst + i * C, acc);
  }
}

template <int C>
static int rs_zoom_launch(const ZoomParams& p, int order, int blocks, hipStream_t stream) {
  (void)hipGetLastError();
  if (order == 0) hipLaunchKernelGGL((rs_zoom_kernel<C, 1>), dim3(blocks), dim3(256), 0, stream, p);
  else if (order == 1) hipLaunchKernelGGL((rs_zoom_kernel<C, 2>), dim3(blocks), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((rs_zoom_kernel<C, 4>), dim3(blocks), dim3(256), 0, stream, p);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_zoom3d(const float* coef, float* dst, float* bmask, const float* mean, const float* stdv, int Din, int Hin,
                          int Win, int Dout, int Hout, int Wout, int C, int Dpad, int Hpad, int Wpad, int order,
                          hipStream_t stream) {
  if (Din < 1 || Hin < 1 || Win < 1 || Dout < 1 || Hout < 1 || Wout < 1 || C < 1 || C > RS_MAXC) return BTS_ERR_SHAPE;
  if (Dpad < Dout || Hpad < Hout || Wpad < Wout) return BTS_ERR_SHAPE;
  if ((mean == nullptr) != (stdv == nullptr)) return BTS_ERR_SHAPE;
  if (order != 0 && order != 1 && order != 3) return BTS_ERR_UNSUPPORTED;
  const uintptr_t amask = (C % 4 == 0) ? 15 : (C == 2 ? 7 : 3);  // whole voxels move as float4 / float2
  if (((uintptr_t)coef | (uintptr_t)dst) & amask) return BTS_ERR_ALIGN;
  ZoomParams p;
  p.coef = coef; p.dst = dst; p.bmask = bmask; p.mean = mean; p.stdv = stdv;
  p.Din = Din; p.Hin = Hin; p.Win = Win; p.Dout = Dout; p.Hout = Hout; p.Wout = Wout; p.Dpad = Dpad; p.Hpad = Hpad; p.Wpad = Wpad;
  p.sd = Dout > 1 ? (double)(Din - 1) / (double)(Dout - 1) : 1.0;
  p.sh = Hout > 1 ? (double)(Hin - 1) / (double)(Hout - 1) : 1.0;
  p.sw = Wout > 1 ? (double)(Win - 1) / (double)(Wout - 1) : 1.0;
  const long total = (long)Dpad * Hpad * Wpad;
  long blocks = (total + 255) / 256;
  if (blocks > 262144) blocks = 262144;
  switch (C) {
    case 1: return rs_zoom_launch<1>(p, order, (int)blocks, stream);
    case 2: return rs_zoom_launch<2>(p, order, (int)blocks, stream);
    case 3: return rs_zoom_launch<3>(p, order, (int)blocks, stream);
    case 4: return rs_zoom_launch<4>(p, order, (int)blocks, stream);
    case 5: return rs_zoom_launch<5>(p, order, (int)blocks, stream);
    case 6: return rs_zoom_launch<6>(p, order, (int)blocks, stream);
    case 7: return rs_zoom_launch<7>(p, order, (int)blocks, stream);
    default: return rs_zoom_launch<8>(p, order, (int)blocks, stream);
  }
}
