// Conforming a scan to an oriented grid by its affine: the two device passes of infer.Conformer.
// Tensors are dense fp32 (D,H,W,C), C innermost, 1 <= C <= 8, as in resample.hip.  All offsets are 64-bit.
//
//   bts_reorient3d          dst = flip(transpose(src)): an exact copy.  Where the output W axis is the source W axis a row of the output
//                           is a row of the source, read forwards or backwards voxel by voxel: a plain gather of whole voxels is coalesced
//                           on both sides.
//                           Where it comes from the source D or H axis that gather would read one voxel per cache line, so a block stages
//                           a tile (TJ source lines of TI voxels) in LDS: it is read along the source W axis and written along the output
//                           W axis, whole runs of whole voxels on either side.
//   bts_affine_resample3d   one thread per output voxel, all C channels in registers: the source coordinate M (o0,o1,o2,1) in fp64 (so
//                           integer-valued maps are exact), then the taps of bts_zoom3d (resample_taps.h; order 1 summed in fp64); 0 outside the source's
//                           field of view [-0.5, n - 0.5] and in the padding; written to channels c0 .. c0+C-1 of a wider destination.
//   bts_label_resample3d    a label map (C = 1) through the same map: the 8 taps of order 1 vote with their fp64 weights, the value with
//                           the largest total wins, of equal totals the smallest (preprocess --conform; nnU-Net's per-class linear
//                           interpolation and arg-max, in one gather).
#include "common.h"
#include "bts_internal.h"
#include "resample_taps.h"

#define CF_TILE_FLOATS 64  // floats of one staged source line: TI = 64 / C voxels, 256 B for C in {1, 2, 4, 8}

struct ReorientParams {
  const float* src;
  float* dst;
  int O0, O1, O2, C;       // output extents
  long base, st0, st1, st2;  // source voxel of output voxel (0,0,0) and the source step of each output axis (negative where reversed)
};

// output W along source W: consecutive threads take consecutive voxels of the output, a voxel's C channels in one access where C allows
template <int C>
__global__ __launch_bounds__(256) void cf_reorient_rows_kernel(const ReorientParams p) {
  const long total = (long)p.O0 * p.O1 * p.O2;
  for (long v = blockIdx.x * 256L + threadIdx.x; v < total; v += (long)gridDim.x * 256L) {
    const long row = v / p.O2;
    const int o2 = (int)(v - row * p.O2);
    const long o0 = row / p.O1, o1 = row - o0 * p.O1;
    float t[C];
    rs_load<C>(p.src + (p.base + o0 * p.st0 + o1 * p.st1 + o2 * p.st2) * C, t);
    rs_store<C>(p.dst + v * C, t);
  }
}

template <int C>
static int cf_rows_launch(const ReorientParams& p, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(cf_reorient_rows_kernel<C>, dim3(blocks), dim3(256), 0, stream, p);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

struct TransposeParams {
  const float* src;
  float* dst;
  int Ni, Nj, Nk;      // source extents: i the source W axis, j the source axis the output W runs along, k the third one
  long sj, sk;         // source strides of j and k in voxels (that of i is 1)
  long oi, ok;         // output strides, in voxels, of the output axes that i and k become (that of j is 1)
  int fi, fj, fk;      // reversed?
  int TI, TJ, pitch;
};

// A tile is TJ source lines (consecutive j) of TI voxels (consecutive i), pitch floats apart in LDS; a thread moves a whole voxel (one
// 16- / 8-byte access for C % 4 == 0 / C == 2: voxels are aligned on both sides wherever the volumes are).  Filling it, the lanes of a wave
// take consecutive voxels of one line.  Emptying it, consecutive lanes take the same voxel column i of consecutive lines, LDS float
// j * pitch + i * C: with pitch % 32 == min(C, 4) for C in {1, 2, 4, 8} the 16 / 32 lanes of one LDS access group cover all 64 banks
// once; for the other C, read float by float, pitch % 32 == C keeps the lanes of a group on distinct banks.
template <int C>
__global__ __launch_bounds__(256) void cf_reorient_tiles_kernel(const TransposeParams p) {
  extern __shared__ __attribute__((aligned(16))) float cf_tile[];
  const long ti = (p.Ni + p.TI - 1) / p.TI, tj = (p.Nj + p.TJ - 1) / p.TJ;
  const long ntiles = ti * tj * p.Nk;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long u = t / ti, k = u / tj;
    const int i0 = (int)(t - u * ti) * p.TI, j0 = (int)(u - k * tj) * p.TJ;
    const int ni = p.Ni - i0 < p.TI ? p.Ni - i0 : p.TI, nj = p.Nj - j0 < p.TJ ? p.Nj - j0 : p.TJ;
    const float* s = p.src + (k * p.sk + (long)j0 * p.sj + i0) * C;
    for (int e = threadIdx.x; e < nj * ni; e += 256) {
      const int j = e / ni, i = e - j * ni;
      float v[C];
      rs_load<C>(s + ((long)j * p.sj + i) * C, v);
      rs_store<C>(cf_tile + j * p.pitch + i * C, v);
    }
    __syncthreads();
    const long ko = p.fk ? p.Nk - 1 - k : k;
    const int w0 = p.fj ? p.Nj - j0 - nj : j0;  // the tile's lines, in output order, are output W positions w0 .. w0 + nj - 1
    float* d = p.dst + (ko * p.ok + w0) * C;
    for (int e = threadIdx.x; e < ni * nj; e += 256) {
      const int i = e / nj, jo = e - i * nj;
      const int j = p.fj ? nj - 1 - jo : jo;
      const long io = p.fi ? p.Ni - 1 - (i0 + i) : i0 + i;
      float v[C];
      rs_load<C>(cf_tile + j * p.pitch + i * C, v);
      rs_store<C>(d + (io * p.oi + jo) * C, v);
    }
    __syncthreads();
  }
}

template <int C>
static int cf_tiles_launch(const TransposeParams& p, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(cf_reorient_tiles_kernel<C>, dim3(blocks), dim3(256), (size_t)p.TJ * p.pitch * sizeof(float), stream, p);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_reorient3d(const float* src, float* dst, int D, int H, int W, int C, int perm0, int perm1, int perm2, int flip_mask,
                              hipStream_t stream) {
  if (D < 1 || H < 1 || W < 1 || C < 1 || C > RS_MAXC) return BTS_ERR_SHAPE;
  const int perm[3] = {perm0, perm1, perm2};
  int seen = 0;
  for (int a = 0; a < 3; ++a) {
    if (perm[a] < 0 || perm[a] > 2) return BTS_ERR_SHAPE;
    seen |= 1 << perm[a];
  }
  if (seen != 7 || flip_mask < 0 || flip_mask > 7) return BTS_ERR_SHAPE;
  if (src == nullptr || dst == nullptr || src == dst) return BTS_ERR_SHAPE;
  const int S[3] = {D, H, W};
  const long sst[3] = {(long)H * W, (long)W, 1L};  // source strides in voxels
  int O[3], flip[3];
  for (int a = 0; a < 3; ++a) {
    O[a] = S[perm[a]];
    flip[a] = (flip_mask >> (2 - a)) & 1;  // bits 4 | 2 | 1 reverse output axis 0 | 1 | 2, as bts_flip_affine counts them
  }
  (void)hipGetLastError();
  const uintptr_t amask = (C % 4 == 0) ? 15 : (C == 2 ? 7 : 3);  // whole voxels move as float4 / float2
  if (((uintptr_t)src | (uintptr_t)dst) & amask) return BTS_ERR_ALIGN;
  if (perm2 == 2) {
    ReorientParams p;
    p.src = src; p.dst = dst; p.O0 = O[0]; p.O1 = O[1]; p.O2 = O[2]; p.C = C;
    long step[3];
    p.base = 0;
    for (int a = 0; a < 3; ++a) {
      step[a] = flip[a] ? -sst[perm[a]] : sst[perm[a]];
      if (flip[a]) p.base += (long)(O[a] - 1) * sst[perm[a]];
    }
    p.st0 = step[0]; p.st1 = step[1]; p.st2 = step[2];
    const long total = (long)D * H * W;
    long blocks = (total + 255) / 256;
    if (blocks > 262144) blocks = 262144;
    switch (C) {
      case 1: return cf_rows_launch<1>(p, (int)blocks, stream);
      case 2: return cf_rows_launch<2>(p, (int)blocks, stream);
      case 3: return cf_rows_launch<3>(p, (int)blocks, stream);
      case 4: return cf_rows_launch<4>(p, (int)blocks, stream);
      case 5: return cf_rows_launch<5>(p, (int)blocks, stream);
      case 6: return cf_rows_launch<6>(p, (int)blocks, stream);
      case 7: return cf_rows_launch<7>(p, (int)blocks, stream);
      default: return cf_rows_launch<8>(p, (int)blocks, stream);
    }
  }
  const int q = perm0 == 2 ? 0 : 1, r = 1 - q;  // the output axes that the source W axis and the third source axis become
  const long ost[3] = {(long)O[1] * O[2], (long)O[2], 1L};
  TransposeParams p;
  p.src = src; p.dst = dst;
  p.Ni = W; p.Nj = S[perm2]; p.Nk = S[perm[r]];
  p.sj = sst[perm2]; p.sk = sst[perm[r]];
  p.oi = ost[q]; p.ok = ost[r];
  p.fi = flip[q]; p.fj = flip[2]; p.fk = flip[r];
  p.TI = CF_TILE_FLOATS / C;
  p.TJ = C <= 2 ? 64 : 32;
  const int tic = p.TI * C, want = C == 8 ? 4 : C;
  p.pitch = tic + (((want - tic) % 32) + 32) % 32;
  long ntiles = (long)((p.Ni + p.TI - 1) / p.TI) * ((p.Nj + p.TJ - 1) / p.TJ) * p.Nk;
  if (ntiles > 262144) ntiles = 262144;
  switch (C) {
    case 1: return cf_tiles_launch<1>(p, (int)ntiles, stream);
    case 2: return cf_tiles_launch<2>(p, (int)ntiles, stream);
    case 3: return cf_tiles_launch<3>(p, (int)ntiles, stream);
    case 4: return cf_tiles_launch<4>(p, (int)ntiles, stream);
    case 5: return cf_tiles_launch<5>(p, (int)ntiles, stream);
    case 6: return cf_tiles_launch<6>(p, (int)ntiles, stream);
    case 7: return cf_tiles_launch<7>(p, (int)ntiles, stream);
    default: return cf_tiles_launch<8>(p, (int)ntiles, stream);
  }
}

struct AffineParams {
  const float* coef;
  float* dst;
  float* bmask;
  int Ds, Hs, Ws, Do, Ho, Wo, Dp, Hp, Wp;
  int ld, c0, vec;  // vec: a voxel's C channels in dst may move as float4 / float2
  double m[12];     // source voxel = m (o0, o1, o2, 1), row-major 3 x 4
};

// order 1 at a general coordinate: the 8 taps in row-major order, weights and sum in fp64, rounded once.  On zoom()'s grid each axis has
// its own fraction and fp32 weights stay within 2 ulp of max|v|; with three arbitrary fractions per voxel the fp32 products alone do not.
template <int C>
__device__ __forceinline__ void cf_trilinear(const float* coef, int Ds, int Hs, int Ws, double sd, double sh, double sw, float* acc) {
  const double fd = floor(sd), fh = floor(sh), fw = floor(sw);
  const int id[2] = {rs_reflect((int)fd, Ds), rs_reflect((int)fd + 1, Ds)};
  const int ih[2] = {rs_reflect((int)fh, Hs), rs_reflect((int)fh + 1, Hs)};
  const int iw[2] = {rs_reflect((int)fw, Ws), rs_reflect((int)fw + 1, Ws)};
  const double wd[2] = {1.0 - (sd - fd), sd - fd}, wh[2] = {1.0 - (sh - fh), sh - fh}, ww[2] = {1.0 - (sw - fw), sw - fw};
  double sum[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sum[c] = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float* row = coef + ((long)id[a] * Hs + ih[b]) * Ws * C;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        float t[C];
        rs_load<C>(row + (long)iw[k] * C, t);
        const double wt = wd[a] * wh[b] * ww[k];
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] += wt * (double)t[c];
      }
    }
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = (float)sum[c];
}

// NT taps per axis: 1 = order 0, 4 = order 3 on prefiltered coefficients (rs_taps_at, rs_accumulate); 2 = order 1 (cf_trilinear)
template <int C, int NT>
__global__ __launch_bounds__(256) void cf_affine_kernel(const AffineParams p) {
  const long total = (long)p.Dp * p.Hp * p.Wp;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    long v = i;
    const int w = (int)(v % p.Wp); v /= p.Wp;
    const int h = (int)(v % p.Hp);
    const int d = (int)(v / p.Hp);
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    if (d < p.Do && h < p.Ho && w < p.Wo) {
      const double od = (double)d, oh = (double)h, ow = (double)w;
      // the translation last, as scipy.ndimage.affine_transform sums it
      const double sd = fma(p.m[2], ow, fma(p.m[1], oh, p.m[0] * od)) + p.m[3];
      const double sh = fma(p.m[6], ow, fma(p.m[5], oh, p.m[4] * od)) + p.m[7];
      const double sw = fma(p.m[10], ow, fma(p.m[9], oh, p.m[8] * od)) + p.m[11];
      // inside the field of view on every axis; a non-finite coordinate is outside
      if (sd >= -0.5 && sd <= (double)p.Ds - 0.5 && sh >= -0.5 && sh <= (double)p.Hs - 0.5 && sw >= -0.5 && sw <= (double)p.Ws - 0.5) {
        if constexpr (NT == 2) {
          cf_trilinear<C>(p.coef, p.Ds, p.Hs, p.Ws, sd, sh, sw, acc);
        } else {
          int id[NT], ih[NT], iw[NT];
          float wd[NT], wh[NT], ww[NT];
          rs_taps_at<NT>(sd, p.Ds, id, wd);
          rs_taps_at<NT>(sh, p.Hs, ih, wh);
          rs_taps_at<NT>(sw, p.Ws, iw, ww);
          rs_accumulate<C, NT>(p.coef, p.Hs, p.Ws, id, ih, iw, wd, wh, ww, acc);
        }
      }
    }
    if (p.bmask) {  // max over channels > 0, as bts_zoom3d forms it
      float mx = acc[0];
#pragma unroll
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, acc[c]);
      p.bmask[i] = mx > 0.f ? 1.f : 0.f;
    }
    float* o = p.dst + i * p.ld + p.c0;
    if (p.vec) {
      rs_store<C>(o, acc);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = acc[c];
    }
  }
}

template <int C>
static int cf_affine_launch(const AffineParams& p, int order, int blocks, hipStream_t stream) {
  (void)hipGetLastError();
  if (order == 0) hipLaunchKernelGGL((cf_affine_kernel<C, 1>), dim3(blocks), dim3(256), 0, stream, p);
  else if (order == 1) hipLaunchKernelGGL((cf_affine_kernel<C, 2>), dim3(blocks), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((cf_affine_kernel<C, 4>), dim3(blocks), dim3(256), 0, stream, p);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" int bts_affine_resample3d(const float* coef, int Ds, int Hs, int Ws, int C, float* dst, int ld_dst, int c0, float* bmask,
                                     int Do, int Ho, int Wo, int Dp, int Hp, int Wp, const double* m12, int order, hipStream_t stream) {
  if (Ds < 1 || Hs < 1 || Ws < 1 || Do < 1 || Ho < 1 || Wo < 1 || C < 1 || C > RS_MAXC) return BTS_ERR_SHAPE;
  if (Dp < Do || Hp < Ho || Wp < Wo) return BTS_ERR_SHAPE;
  if (ld_dst < C || c0 < 0 || c0 + C > ld_dst) return BTS_ERR_SHAPE;
  if (coef == nullptr || dst == nullptr || m12 == nullptr) return BTS_ERR_SHAPE;
  if (bmask != nullptr && (c0 != 0 || ld_dst != C)) return BTS_ERR_SHAPE;  // the mask is the maximum over ALL channels of the volume
  if (order != 0 && order != 1 && order != 3) return BTS_ERR_UNSUPPORTED;
  const uintptr_t amask = (C % 4 == 0) ? 15 : (C == 2 ? 7 : 3);  // whole voxels of coef are read as float4 / float2
  if ((uintptr_t)coef & amask) return BTS_ERR_ALIGN;
  if ((uintptr_t)dst & 3) return BTS_ERR_ALIGN;
  AffineParams p;
  p.coef = coef; p.dst = dst; p.bmask = bmask;
  p.Ds = Ds; p.Hs = Hs; p.Ws = Ws; p.Do = Do; p.Ho = Ho; p.Wo = Wo; p.Dp = Dp; p.Hp = Hp; p.Wp = Wp;
  p.ld = ld_dst; p.c0 = c0;
  const int lanes = (C % 4 == 0) ? 4 : (C == 2 ? 2 : 1);
  p.vec = (((uintptr_t)(dst + c0) & amask) == 0 && ld_dst % lanes == 0) ? 1 : 0;
  for (int k = 0; k < 12; ++k) p.m[k] = m12[k];
  const long total = (long)Dp * Hp * Wp;
  long blocks = (total + 255) / 256;
  if (blocks > 262144) blocks = 262144;
  switch (C) {
    case 1: return cf_affine_launch<1>(p, order, (int)blocks, stream);
    case 2: return cf_affine_launch<2>(p, order, (int)blocks, stream);
    case 3: return cf_affine_launch<3>(p, order, (int)blocks, stream);
    case 4: return cf_affine_launch<4>(p, order, (int)blocks, stream);
    case 5: return cf_affine_launch<5>(p, order, (int)blocks, stream);
    case 6: return cf_affine_launch<6>(p, order, (int)blocks, stream);
    case 7: return cf_affine_launch<7>(p, order, (int)blocks, stream);
    default: return cf_affine_launch<8>(p, order, (int)blocks, stream);
  }
}

struct LabelParams {
  const float* lab;
  float* dst;
  int Ds, Hs, Ws, Do, Ho, Wo, Dp, Hp, Wp;
  double m[12];  // as AffineParams
};

// A label map through the same map: the coordinate, the field of view and the 8 taps (indices, fp64 weights (wd * wh) * ww, row-major
// order) of cf_affine_kernel<1, 2> / cf_trilinear, but the taps vote instead of being summed.  A label value's weight is the sum, in tap
// order, of the weights of the taps that hold it; every tap's value gets its total by comparing it with all 8 (taps of one value get the
// same sum, term for term), the largest total wins and of equal totals the smallest value.  All in registers, for any values.
__global__ __launch_bounds__(256) void cf_label_kernel(const LabelParams p) {
  const long total = (long)p.Dp * p.Hp * p.Wp;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    long v = i;
    const int w = (int)(v % p.Wp); v /= p.Wp;
    const int h = (int)(v % p.Hp);
    const int d = (int)(v / p.Hp);
    float res = 0.f;
    if (d < p.Do && h < p.Ho && w < p.Wo) {
      const double od = (double)d, oh = (double)h, ow = (double)w;
      const double sd = fma(p.m[2], ow, fma(p.m[1], oh, p.m[0] * od)) + p.m[3];
      const double sh = fma(p.m[6], ow, fma(p.m[5], oh, p.m[4] * od)) + p.m[7];
      const double sw = fma(p.m[10], ow, fma(p.m[9], oh, p.m[8] * od)) + p.m[11];
      if (sd >= -0.5 && sd <= (double)p.Ds - 0.5 && sh >= -0.5 && sh <= (double)p.Hs - 0.5 && sw >= -0.5 && sw <= (double)p.Ws - 0.5) {
        const double fd = floor(sd), fh = floor(sh), fw = floor(sw);
        const int id[2] = {rs_reflect((int)fd, p.Ds), rs_reflect((int)fd + 1, p.Ds)};
        const int ih[2] = {rs_reflect((int)fh, p.Hs), rs_reflect((int)fh + 1, p.Hs)};
        const int iw[2] = {rs_reflect((int)fw, p.Ws), rs_reflect((int)fw + 1, p.Ws)};
        const double wd[2] = {1.0 - (sd - fd), sd - fd}, wh[2] = {1.0 - (sh - fh), sh - fh}, ww[2] = {1.0 - (sw - fw), sw - fw};
        float val[8];
        double wt[8];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const float* row = p.lab + ((long)id[a] * p.Hs + ih[b]) * p.Ws;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              val[4 * a + 2 * b + k] = row[iw[k]];
              wt[4 * a + 2 * b + k] = wd[a] * wh[b] * ww[k];
            }
          }
        double best = -1.0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          double sum = 0.0;
#pragma unroll
          for (int u = 0; u < 8; ++u) sum += val[u] == val[t] ? wt[u] : 0.0;
          if (sum > best || (sum == best && val[t] < res)) {
            best = sum;
            res = val[t];
          }
        }
      }
    }
    p.dst[i] = res;
  }
}

extern "C" int bts_label_resample3d(const float* lab, int Ds, int Hs, int Ws, float* dst, int Do, int Ho, int Wo, int Dp, int Hp, int Wp,
                                    const double* m12, hipStream_t stream) {
  if (Ds < 1 || Hs < 1 || Ws < 1 || Do < 1 || Ho < 1 || Wo < 1) return BTS_ERR_SHAPE;
  if (Dp < Do || Hp < Ho || Wp < Wo) return BTS_ERR_SHAPE;
  if (lab == nullptr || dst == nullptr || m12 == nullptr || lab == dst) return BTS_ERR_SHAPE;
  if (((uintptr_t)lab | (uintptr_t)dst) & 3) return BTS_ERR_ALIGN;
  LabelParams p;
  p.lab = lab; p.dst = dst;
  p.Ds = Ds; p.Hs = Hs; p.Ws = Ws; p.Do = Do; p.Ho = Ho; p.Wo = Wo; p.Dp = Dp; p.Hp = Hp; p.Wp = Wp;
  for (int k = 0; k < 12; ++k) p.m[k] = m12[k];
  const long total = (long)Dp * Hp * Wp;
  long blocks = (total + 255) / 256;
  if (blocks > 262144) blocks = 262144;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cf_label_kernel, dim3(blocks), dim3(256), 0, stream, p);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
