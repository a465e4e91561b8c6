// 3x3x3 stride-1 conv of a TWO-channel input (the network's first convolutions, model.py / resnet.py:30-37 on the 2ch x 128^3
// volume) into <= 32 output channels.  The tiled kernel pads the 2 channels to a k-group of 8 and runs at a quarter of the
// useful rate; here the contraction index of the MFMA (K = 2) IS the channel pair: one matrix instruction per tap, its B
// operand a single ds_read_b32 of the planar LDS halo tile [channel][z][y][x] (lane = (channel, x)), its A operand the
// tap's 2 x 32 weights held in a register for the whole workgroup.  A wave owns one z plane of the 32 x 4 x 4 tile: the
// 18 input fragments of a kz slab feed the 36 matrix instructions of its four output rows.  Optional second output
// (the 1x1x1 shortcut conv of the same input: one more instruction on the centre fragment), bias, GroupNorm partials.
#include <stdlib.h>
#include "common.h"
#include "conv_plan.h"

struct C2Params {
  const float* x;
  const float* wp;    // K3S1 forward image (KG = 1): W[t][c][n] = wp[(t*2*Npad + n)*4 + c]
  const float* bias;
  float* y;
  const float* wp2;   // K1 forward image of the shortcut (or null): W2[c][n] = wp2[n*4 + c]
  const float* bias2;
  float* y2;
  int N, D, H, W, ldx, Cout, ldy, ldy2, Npad;
  int ntz, nty, ntx;
  double* gnp;
  int gn_G, gn_zt;
};

template <bool F2>
__global__ __launch_bounds__(256, 2) void c2_kernel(const C2Params p) {
  __shared__ float lds[2 * 6 * 6 * 34 + 16];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  int b = blockIdx.x;
  const int tx = b % p.ntx; b /= p.ntx;
  const int ty = b % p.nty; b /= p.nty;
  const int tz = b % p.ntz;
  const int n = b / p.ntz;
  const int oz0 = tz * 4, oy0 = ty * 4, ox0 = tx * 32;
  // ---- halo tile (34 x 6 x 6 voxels x 2 channels) -> planar LDS ----
  for (int e = tid; e < 6 * 6 * 34; e += 256) {
    const int vz = e / (6 * 34), r = e - vz * (6 * 34);
    const int vy = r / 34, vx = r - vy * 34;
    const int z = oz0 - 1 + vz, yy = oy0 - 1 + vy, xx = ox0 - 1 + vx;
    float v0 = 0.f, v1 = 0.f;
    if ((unsigned)z < (unsigned)p.D && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W) {
      const float* s = p.x + ((((long)n * p.D + z) * p.H + yy) * p.W + xx) * (long)p.ldx;
      v0 = s[0]; v1 = s[1];
    }
    lds[e] = v0;
    lds[6 * 6 * 34 + e] = v1;
  }
  // ---- weights: lane (channel h, cout l32) ----
  float wt[27];
#pragma unroll
  for (int t = 0; t < 27; ++t) wt[t] = p.wp[((long)t * 2 * p.Npad + l32) * 4 + h];
  float w2 = 0.f;
  if (F2) w2 = p.wp2[l32 * 4 + h];
  __syncthreads();
  f32x16 acc[4], acc2[F2 ? 4 : 1];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; if (F2) acc2[F2 ? i : 0][r] = 0.f; }
  const float* lb = lds + h * (6 * 6 * 34) + (wave * 6) * 34 + l32;   // (channel h, z = wave + kz, y, x = l32 + kx)
#pragma unroll
  for (int kz = 0; kz < 3; ++kz) {
    float f[6][3];
#pragma unroll
    for (int yr = 0; yr < 6; ++yr)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) f[yr][kx] = lb[(kz * 6 + yr) * 34 + kx];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int oy = 0; oy < 4; ++oy)
          acc[oy] = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[(kz * 3 + ky) * 3 + kx], f[oy + ky][kx], acc[oy], 0, 0, 0);
    if (F2 && kz == 1) {
#pragma unroll
      for (int oy = 0; oy < 4; ++oy) acc2[F2 ? oy : 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2, f[oy + 1][1], acc2[F2 ? oy : 0], 0, 0, 0);
    }
  }
  // ---- epilogue: D rows = couts (4 per register quad), cols = x ----
  const int oz = oz0 + wave, ox = ox0 + l32;
  float gn_s = 0.f, gn_q = 0.f;
  if (oz < p.D && ox < p.W) {
#pragma unroll
    for (int oy = 0; oy < 4; ++oy) {
      const int y = oy0 + oy;
      if (y >= p.H) continue;
      const long pix = (((long)n * p.D + oz) * p.H + y) * p.W + ox;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co = 8 * g + 4 * h;
        if (co >= p.Cout) continue;
        f32x4 v = {acc[oy][4 * g], acc[oy][4 * g + 1], acc[oy][4 * g + 2], acc[oy][4 * g + 3]};
        if (p.bias) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += p.bias[co + j];
        }
        if (p.gnp) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { gn_s += v[j]; gn_q = fmaf(v[j], v[j], gn_q); }
        }
        *reinterpret_cast<f32x4*>(p.y + pix * p.ldy + co) = v;
        if (F2) {
          f32x4 v2 = {acc2[F2 ? oy : 0][4 * g], acc2[F2 ? oy : 0][4 * g + 1], acc2[F2 ? oy : 0][4 * g + 2], acc2[F2 ? oy : 0][4 * g + 3]};
          if (p.bias2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v2[j] += p.bias2[co + j];
          }
          *reinterpret_cast<f32x4*>(p.y2 + pix * p.ldy2 + co) = v2;
        }
      }
    }
  }
  if (p.gnp) {  // fixed-order combine, layout as igemm_kernel's
    const double ds = wave_sum_f64((double)gn_s), dq = wave_sum_f64((double)gn_q);
    __syncthreads();
    double* sh = reinterpret_cast<double*>(lds);
    if (lane == 0) { sh[wave * 2] = ds; sh[wave * 2 + 1] = dq; }
    __syncthreads();
    if (tid == 0) {
      const int g = tz / p.gn_zt;
      const long B = (long)p.gn_zt * p.nty * p.ntx;
      const long b_ = ((long)(tz - g * p.gn_zt) * p.nty + ty) * p.ntx + tx;
      double* o = p.gnp + (((long)n * p.gn_G + g) * B + b_) * 2;
      o[0] = sh[0] + sh[2] + sh[4] + sh[6];
      o[1] = sh[1] + sh[3] + sh[5] + sh[7];
    }
  }
}

// the grid of 32 x 4 x 4 voxel tiles, one workgroup each; returns their number
static inline long c2_tiles(const ConvCall& c, int& ntx, int& nty, int& ntz) {
  ntx = (c.Wi + 31) / 32; nty = (c.Hi + 3) / 4; ntz = (c.Di + 3) / 4;
  return (long)c.N * ntz * nty * ntx;
}
// The two-channel kernel takes plain 3x3x3 calls (bias at most) into <= 32 channels on 16-byte output rows, with or without the fused
// shortcut output, when the grid is worth it; it writes the GroupNorm partials where the slab groups hold whole 4-plane tiles.
bool c2_accept(const ConvCall& c, ConvChoice& ch) {
  if (c.Cin != 2 || c.Cout > 32 || c.Cout % 4 != 0 || c.ldy % 4 != 0 || !c.y16) return false;
  if (c.flags & (IG_FLAG_ACCUM | IG_FLAG_SIGMOID)) return false;
  if (c.second == CONV_Y2 && (c.ld2 % 4 != 0 || !c.p2_16)) return false;
  int ntx, nty, ntz;
  const long tiles = c2_tiles(c, ntx, nty, ntz);
  if (tiles < conv_env_long("BTS_IGEMM_C2_MIN", 512) || tiles > 0x7fffffffL) return false;  // (tests force 1)
  ch.sym = SYM_C2;
  ch.gn_B = (long)conv_gn_zt(c, 4) * nty * ntx;
  return true;
}
int bts_c2_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
  const bool f2 = c.second == CONV_Y2;
  C2Params p;
  p.x = q.x; p.wp = q.wp; p.bias = (c.flags & IG_FLAG_BIAS) ? q.bias : nullptr; p.y = q.y;
  p.wp2 = f2 ? q.wp2 : nullptr; p.bias2 = f2 ? q.bias2 : nullptr; p.y2 = f2 ? q.y2 : nullptr;
  p.N = c.N; p.D = c.Di; p.H = c.Hi; p.W = c.Wi; p.ldx = c.ldx; p.Cout = c.Cout; p.ldy = c.ldy; p.ldy2 = f2 ? c.ld2 : 0; p.Npad = conv_npad32(c.Cout);
  const long tiles = c2_tiles(c, p.ntx, p.nty, p.ntz);
  p.gnp = ch.gn_B ? q.gnp : nullptr; p.gn_G = ch.gn_B ? c.G : 0; p.gn_zt = ch.gn_B ? (c.Di / c.G) / 4 : 1;
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(ch.sym, 2.0 * (27.0 + (f2 ? 1.0 : 0.0)) * c.Cin * (double)c.Cout * (double)c.N * c.Di * c.Hi * c.Wi, stream);
  (void)hipGetLastError();
  if (f2) hipLaunchKernelGGL(c2_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(c2_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
