// 1x1x1, stride-2 and transposed convolutions on 16-bit storage (and the data gradients on those geometries): the two gather kernels and the
// host side of the family -- lp_g_choose (lowp_common.h), the launch of what was chosen, the fused entry points (other kernels: lowp_k1 | s2t | up.hip)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <limits.h>
#include "common.h"
#include "bts_internal.h"
#include "lowp_common.h"

// gather-form convolution (out[o*os+oo] = sum_t in[o*s+off_t] W[t], the transposed conv as 8 output-parity classes): operands straight
// from global memory -- every input voxel is needed by at most 8 outputs, an LDS tile would buy nothing
struct LpTap { short dz, dy, dx, w; };   // input offset of the tap, index of its weight slab
struct LpGatherParams {
  const unsigned short* x;
  const unsigned short* wp;
  const float* bias;
  unsigned short* y;
  int N, Di, Hi, Wi, ldx;           // input grid
  int Dg, Hg, Wg;                   // grid of this launch (output positions of one class)
  int Do, Ho, Wo, ldy, Cout;        // output tensor
  int s, os, ooz, ooy, oox;         // in = g*s + off_t ; out = g*os + oo
  int KS, NB, ncg, ntaps, accum;
  long npos;                        // N*Dg*Hg*Wg
  double* gap_part;                 // fused global-average-pool partials [position block][Cout] (1x1x1 launches only), else NULL
  LpTap taps[27];
};

template <typename T, int VB, int CB>
__global__ __launch_bounds__(256, 2) void lp_conv_gather_kernel(const LpGatherParams p) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int h = lane >> 5, l32 = lane & 31;
  const int cg = blockIdx.x % p.ncg;
  const long blk = blockIdx.x / p.ncg;
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, 0x7fffffff, 0x00020000);
  const unsigned wlane = (unsigned)((h * 32 + l32) * 16);
  // this lane's VB grid positions
  int gz[VB], gy[VB], gx[VB], gn[VB];
  bool live[VB];
#pragma unroll
  for (int v = 0; v < VB; ++v) {
    long pos = ((blk * 4 + wave) * VB + v) * 32 + l32;
    live[v] = pos < p.npos;
    if (!live[v]) pos = 0;
    gx[v] = (int)(pos % p.Wg); pos /= p.Wg;
    gy[v] = (int)(pos % p.Hg); pos /= p.Hg;
    gz[v] = (int)(pos % p.Dg);
    gn[v] = (int)(pos / p.Dg);
  }
  f32x16 acc[VB][CB];
#pragma unroll
  for (int v = 0; v < VB; ++v)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[v][c][r] = 0.f;
  // Software pipeline over the flattened (tap, k-step) sequence: the operands of step i+1 are requested before the matrix
  // instructions of step i run (both operands come straight from global memory: a step without its successor in flight
  // would wait a full memory round trip for every 4-8 matrix instructions)
  const unsigned short* src[VB];   // of the tap being REQUESTED
  bool ok[VB];
  int wtap = 0;
  auto tap_setup = [&](int t) {
    const LpTap tp = p.taps[t];
    wtap = tp.w;
#pragma unroll
    for (int v = 0; v < VB; ++v) {
      const int iz = gz[v] * p.s + tp.dz, iy = gy[v] * p.s + tp.dy, ix = gx[v] * p.s + tp.dx;
      ok[v] = live[v] && (unsigned)iz < (unsigned)p.Di && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
      src[v] = p.x + ((((long)gn[v] * p.Di + iz) * p.Hi + iy) * p.Wi + ix) * (long)p.ldx + h * 8;
    }
  };
  auto request = [&](int ks, u32x4 (&a)[CB], u32x4 (&b)[VB]) {
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int cb = cg * CB + c;
      a[c] = bload16(wr, wlane, (unsigned)((((wtap * p.KS + ks) * p.NB) + (cb < p.NB ? cb : 0)) * 1024));
    }
#pragma unroll
    for (int v = 0; v < VB; ++v) {
      b[v] = u32x4{0u, 0u, 0u, 0u};
      if (ok[v]) b[v] = *reinterpret_cast<const u32x4*>(src[v] + ks * 16);
    }
  };
  // ring of GD + 1 operand sets: step i computes on set i % (GD + 1) while the requests of steps i+1 .. i+GD are in flight
  constexpr int GD = (VB + CB >= 6) ? 2 : 3;   // (4 x 2 tiles: a third set in flight would spill)
  u32x4 ar[GD + 1][CB], br[GD + 1][VB];
  const int total = p.ntaps * p.KS;
  int rt = 0, rks = 0, issued = 0;
  tap_setup(0);
  auto issue = [&](u32x4 (&a)[CB], u32x4 (&b)[VB]) {   // request the operands of step `issued` (no-op past the end)
    if (issued < total) {
      request(rks, a, b);
      ++issued;
      if (++rks == p.KS) { rks = 0; if (++rt < p.ntaps) tap_setup(rt); }
    }
  };
#pragma unroll
  for (int j = 0; j < GD; ++j) issue(ar[j], br[j]);
  for (int i0 = 0; i0 < total; i0 += GD + 1) {
#pragma unroll
    for (int j = 0; j <= GD; ++j) {
      if (i0 + j < total) {
        issue(ar[(j + GD) % (GD + 1)], br[(j + GD) % (GD + 1)]);
#pragma unroll
        for (int v = 0; v < VB; ++v)
#pragma unroll
          for (int c = 0; c < CB; ++c) acc[v][c] = T::mfma(ar[j][c], br[j][v], acc[v][c]);
      }
    }
  }
  float csum[CB][16];   // column sums of what this lane stores (dead code unless p.gap_part)
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) csum[c][r] = 0.f;
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    const int cb = cg * CB + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = cb * 32 + 8 * q + 4 * h;
      float bq[4] = {0.f, 0.f, 0.f, 0.f};
      if (p.bias && cb < p.NB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (co + j < p.Cout) bq[j] = p.bias[co + j];
      }
#pragma unroll
      for (int v = 0; v < VB; ++v) {
        if (live[v] && cb < p.NB && co < p.Cout) {
          const int oz = gz[v] * p.os + p.ooz, oy = gy[v] * p.os + p.ooy, ox = gx[v] * p.os + p.oox;
          if (oz < p.Do && oy < p.Ho && ox < p.Wo) {
            unsigned short* dst = p.y + ((((long)gn[v] * p.Do + oz) * p.Ho + oy) * p.Wo + ox) * (long)p.ldy + co;
            const float o0 = acc[v][c][4 * q] + bq[0], o1 = acc[v][c][4 * q + 1] + bq[1], o2 = acc[v][c][4 * q + 2] + bq[2],
                        o3 = acc[v][c][4 * q + 3] + bq[3];
            lp_store_quad<T>(dst, o0, o1, o2, o3, p.Cout - co, p.accum);
            csum[c][4 * q] += o0; csum[c][4 * q + 1] += o1; csum[c][4 * q + 2] += o2; csum[c][4 * q + 3] += o3;
          }
        }
      }
    }
  }
  // Fused global average pool of the output (resnet.py:121: the squeeze of the block's 1x1x1 shortcut output): column sums of
  // this block's 128 * VB positions -- lanes (xor shuffles over the 32 positions of a wave), the 4 waves through LDS in fixed
  // order, one fp64 partial per (position block, cout); bts_lp_conv1_gap's finalize adds the blocks of a sample
  if (p.gap_part != nullptr) {   // (launch-uniform)
    __shared__ float csh[4][CB * 32];
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = csum[c][r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (l32 == 0) csh[wave][c * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = v;
      }
    __syncthreads();
    if (tid < CB * 32) {
      const int co = cg * CB * 32 + tid;
      if (co < p.Cout) p.gap_part[blk * p.Cout + co] = ((double)csh[0][tid] + (double)csh[1][tid]) + ((double)csh[2][tid] + (double)csh[3][tid]);
    }
  }
}

// Stride-2 gather with whole-row loads.  In the kernel above a B operand is 16 bytes of each of 32 voxels that sit two rows apart:
// an instruction touches 32 cache lines and uses 32 bytes of each, every line comes back for the other k-steps, and the L2 -> L1 fill
// rate bounds the launch (0.09 of the matrix peak at 32 channels).  Here the k-steps of a tap go in groups of GK = 2 | 4 (64 | 128
// bytes of a voxel's row): load instruction i has the GK lanes of a quad fetch the GK * 32 contiguous bytes of output voxel
// (quad base + i), the quad transpose (lowp_common.h) hands every lane its own voxel's pieces, one per k-step.  Two register sets:
// the next group's rows and weight fragments are in flight while the current group multiplies.  Needs Wg % GK == 0 (a quad never
// leaves its output row).
// VB = 4 (round 5): four position groups per wave share every weight fragment -- a wave's weight re-streaming from L2 (one fragment per
// two matrix instructions at VB = 2, as much traffic as the activations) halves; GK = 2 only (register budget: 128 accumulators + two
// operand sets).
template <typename T, int CB, int GK, int VB = 2>
__global__ __launch_bounds__(256, VB == 4 ? 1 : 2) void lp_conv_gatherq_kernel(const LpGatherParams p) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int h = lane >> 5, l32 = lane & 31, b = l32 & (GK - 1);
  const int cg = blockIdx.x % p.ncg;
  const long blk = blockIdx.x / p.ncg;
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, 0x7fffffff, 0x00020000);
  const unsigned wlane = (unsigned)((h * 32 + l32) * 16);
  int gz[VB], gy[VB], gx[VB], gn[VB];
  bool live[VB];
  const unsigned short* base[VB];     // own voxel's quad base (n, s gz, s gy, s (gx - b)), this lane's piece of a chunk
#pragma unroll
  for (int v = 0; v < VB; ++v) {
    long pos = ((blk * 4 + wave) * VB + v) * 32 + l32;
    live[v] = pos < p.npos;           // (npos is a multiple of Wg, Wg of GK: the lanes of a quad are live together)
    if (!live[v]) pos = 0;
    gx[v] = (int)(pos % p.Wg); pos /= p.Wg;
    gy[v] = (int)(pos % p.Hg); pos /= p.Hg;
    gz[v] = (int)(pos % p.Dg);
    gn[v] = (int)(pos / p.Dg);
    base[v] = p.x + ((((long)gn[v] * p.Di + gz[v] * p.s) * p.Hi + gy[v] * p.s) * p.Wi + (long)(gx[v] - b) * p.s) * (long)p.ldx + (2 * b + h) * 8;
  }
  f32x16 acc[VB][CB];
#pragma unroll
  for (int v = 0; v < VB; ++v)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[v][c][r] = 0.f;
  const int NQ = p.KS / GK;                 // chunks per tap
  const int total = p.ntaps * NQ;
  int rt = 0, rq = 0, issued = 0;
  u32x4 a0[GK][CB], a1[GK][CB], b0[VB][GK], b1[VB][GK];
  auto issue = [&](u32x4 (&a)[GK][CB], u32x4 (&bb)[VB][GK]) {
    if (issued >= total) return;
    const LpTap tp = p.taps[rt];
#pragma unroll
    for (int j = 0; j < GK; ++j)
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const int cb = cg * CB + c;
        a[j][c] = bload16(wr, wlane, (unsigned)((((tp.w * p.KS + rq * GK + j) * p.NB) + (cb < p.NB ? cb : 0)) * 1024));
      }
    const long off = (((long)tp.dz * p.Hi + tp.dy) * p.Wi + tp.dx) * (long)p.ldx + rq * (GK * 16);
#pragma unroll
    for (int v = 0; v < VB; ++v) {
      const int iz = gz[v] * p.s + tp.dz, iy = gy[v] * p.s + tp.dy;
      const bool okzy = live[v] && (unsigned)iz < (unsigned)p.Di && (unsigned)iy < (unsigned)p.Hi;
#pragma unroll
      for (int i = 0; i < GK; ++i) {
        const int ix = (gx[v] - b + i) * p.s + tp.dx;
        bb[v][i] = u32x4{0u, 0u, 0u, 0u};
        if (okzy && (unsigned)ix < (unsigned)p.Wi) bb[v][i] = *reinterpret_cast<const u32x4*>(base[v] + off + (long)i * p.s * p.ldx);
      }
    }
    ++issued;
    if (++rq == NQ) { rq = 0; ++rt; }
  };
  auto compute = [&](u32x4 (&a)[GK][CB], u32x4 (&bb)[VB][GK]) {
#pragma unroll
    for (int v = 0; v < VB; ++v) {
      if constexpr (GK == 4) k1_quad_transpose(bb[v], b); else k1_pair_transpose(bb[v], b);
    }
#pragma unroll
    for (int j = 0; j < GK; ++j)
#pragma unroll
      for (int v = 0; v < VB; ++v)
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[v][c] = T::mfma(a[j][c], bb[v][j], acc[v][c]);
  };
  issue(a0, b0);
  for (int g = 0; g < total; g += 2) {
    issue(a1, b1);
    compute(a0, b0);
    if (g + 1 < total) {
      issue(a0, b0);
      compute(a1, b1);
    }
  }
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    const int cb = cg * CB + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = cb * 32 + 8 * q + 4 * h;
      float bq[4] = {0.f, 0.f, 0.f, 0.f};
      if (p.bias && cb < p.NB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (co + j < p.Cout) bq[j] = p.bias[co + j];
      }
#pragma unroll
      for (int v = 0; v < VB; ++v) {
        if (live[v] && cb < p.NB && co < p.Cout) {
          const int oz = gz[v] * p.os + p.ooz, oy = gy[v] * p.os + p.ooy, ox = gx[v] * p.os + p.oox;
          if (oz < p.Do && oy < p.Ho && ox < p.Wo) {
            unsigned short* dst = p.y + ((((long)gn[v] * p.Do + oz) * p.Ho + oy) * p.Wo + ox) * (long)p.ldy + co;
            lp_store_quad<T>(dst, acc[v][c][4 * q] + bq[0], acc[v][c][4 * q + 1] + bq[1], acc[v][c][4 * q + 2] + bq[2], acc[v][c][4 * q + 3] + bq[3],
                             p.Cout - co, p.accum);
          }
        }
      }
    }
  }
}

// The gather kernels take every call of the family: plain form on tiles of 128 * vb positions x cb cout blocks, or -- stride 2 on grids
// that fill the chip -- whole-row loads.  They write the squeeze's partial rows for dense y and samples that are whole position blocks.
bool lp_gather_accept(const LpGCall& c, LpGChoice& ch) {
  LpGatherPlan& g = ch.g;
  const bool s2 = c.geo == 2;
  const int Dg = s2 ? (c.D + 1) / 2 : c.D, Hg = s2 ? (c.H + 1) / 2 : c.H, Wg = s2 ? (c.W + 1) / 2 : c.W;
  const int KS = c.Cin / 16, NB = (c.Cout + 31) / 32;
  const long V = (long)Dg * Hg * Wg;
  g.npos = c.N * V;
  g.cb = NB >= 2 ? 2 : 1;
  g.ncg = (NB + g.cb - 1) / g.cb;
  const long wg4 = ((g.npos + 511) / 512) * g.ncg;
  g.vb = wg4 >= 512 ? 4 : (wg4 >= 128 ? 2 : 1);
  // whole-row loads for the stride-2 forms on grids that fill the chip (BTS_LP_GATHERQ=0: the plain kernel, for A/B; read per call)
  g.gk = 0;
  if (lp_switch_on("BTS_LP_GATHERQ") && s2 && g.vb >= 2 && KS % 2 == 0) {
    if (KS % 4 == 0 && Wg % 4 == 0) g.gk = 4;
    else if (Wg % 2 == 0) g.gk = 2;
  }
  // (below ~300 workgroups the plain kernel's smaller tiles win: 128 -> 128 at 8 x 32^3, 256 workgroups, 77 against 90 us)
  { const char* m = getenv("BTS_LP_GATHERQ_MIN"); if (g.gk && ((g.npos + 255) / 256) * g.ncg < (m ? atol(m) : 288)) g.gk = 0; }
  if (g.gk) {
    // four position groups per wave: OFF by default -- measured in round 5 (profiles/r05_ab_e6_gatherq_vb4.txt): the 128 accumulators
    // + two operand sets need 442 registers, i.e. one wave per SIMD, and the batch-8 step loses 1.7 ms (76.6 against 74.9), the
    // inference forward nothing / 0.1 ms.  BTS_LP_GATHERQ_VB4=<n> (n > 1) takes grids of at least n double-size workgroups (tests, A/B)
    const char* v4 = getenv("BTS_LP_GATHERQ_VB4");
    const bool vb4 = v4 && atoi(v4) > 1 && g.cb == 2 && Wg % 2 == 0 && ((g.npos + 511) / 512) * g.ncg >= atol(v4);
    g.vb = vb4 ? 4 : 2;
    if (vb4) g.gk = 2;
  }
  g.blocks = ((g.npos + 128L * g.vb - 1) / (128L * g.vb)) * g.ncg;
  if (c.want_gap && c.ldy == c.Cout && V % (128L * g.vb) == 0) ch.rows = V / (128L * g.vb);
  return g.blocks <= 0x7fffffffL;      // (else more workgroups than a grid holds)
}
template <typename T>
static int lp_gather_launch(const LpGatherParams& p, const LpGatherPlan& g, hipStream_t stream) {
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(31, 2.0 * p.ntaps * 16.0 * p.KS * p.Cout * (double)p.npos, stream);
  (void)hipGetLastError();
  const dim3 grid((unsigned)g.blocks);
  if (g.gk) {
#define LP_GQ(CB_, GK_) hipLaunchKernelGGL((lp_conv_gatherq_kernel<T, CB_, GK_>), grid, dim3(256), 0, stream, p)
    if (g.vb == 4) hipLaunchKernelGGL((lp_conv_gatherq_kernel<T, 2, 2, 4>), grid, dim3(256), 0, stream, p);
    else if (g.cb == 2) { if (g.gk == 4) LP_GQ(2, 4); else LP_GQ(2, 2); }
    else { if (g.gk == 4) LP_GQ(1, 4); else LP_GQ(1, 2); }
#undef LP_GQ
  } else {
#define LP_G_CASE(VB_, CB_) if (g.vb == VB_ && g.cb == CB_) hipLaunchKernelGGL((lp_conv_gather_kernel<T, VB_, CB_>), grid, dim3(256), 0, stream, p);
    LP_G_CASE(4, 1) LP_G_CASE(4, 2) LP_G_CASE(2, 1) LP_G_CASE(2, 2) LP_G_CASE(1, 1) LP_G_CASE(1, 2)
#undef LP_G_CASE
  }
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
// the tap tables of the three geometries, and the launch (the transposed form: one per output-parity class)
static int lp_gather_run(int dtype, const LpGCall& c, const LpGChoice& ch, const LpGPtrs& q, hipStream_t stream) {
  LpGatherParams g;
  g.x = (const unsigned short*)q.x; g.wp = (const unsigned short*)q.wp; g.bias = q.bias; g.y = (unsigned short*)q.y;
  g.N = c.N; g.Di = c.D; g.Hi = c.H; g.Wi = c.W; g.ldx = c.ldx; g.ldy = c.ldy; g.Cout = c.Cout; g.KS = c.Cin / 16; g.NB = (c.Cout + 31) / 32;
  g.accum = c.accum; g.ncg = ch.g.ncg; g.npos = ch.g.npos; g.gap_part = q.part;
  auto run = [&]() { return lp_typed(dtype, [&](auto t) { return lp_gather_launch<decltype(t)>(g, ch.g, stream); }); };
  if (c.geo == 0) {
    g.Dg = g.Do = c.D; g.Hg = g.Ho = c.H; g.Wg = g.Wo = c.W; g.s = 1; g.os = 1; g.ooz = g.ooy = g.oox = 0; g.ntaps = 1;
    g.taps[0] = LpTap{0, 0, 0, 0};
    return run();
  }
  if (c.geo == 2) {   // TF 'same', stride 2: out = ceil(in/2), pad_before = max((out-1)*2+3-in, 0) / 2
    g.Do = (c.D + 1) / 2; g.Ho = (c.H + 1) / 2; g.Wo = (c.W + 1) / 2;
    g.Dg = g.Do; g.Hg = g.Ho; g.Wg = g.Wo; g.s = 2; g.os = 1; g.ooz = g.ooy = g.oox = 0; g.ntaps = 27;
    auto padb = [](int in, int out) { const int t = (out - 1) * 2 + 3 - in; return t > 0 ? t / 2 : 0; };
    const int pz = padb(c.D, g.Do), py = padb(c.H, g.Ho), px = padb(c.W, g.Wo);
    for (int t = 0; t < 27; ++t) g.taps[t] = LpTap{(short)(t / 9 - pz), (short)((t / 3) % 3 - py), (short)(t % 3 - px), (short)t};
    return run();
  }
  // y[2i+k] += x[i] w[k], cropped to [0, 2n): 8 output-parity classes, every output written once
  g.Do = 2 * c.D; g.Ho = 2 * c.H; g.Wo = 2 * c.W; g.Dg = c.D; g.Hg = c.H; g.Wg = c.W; g.s = 1; g.os = 2;
  for (int cls = 0; cls < 8; ++cls) {
    const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
    int ozs[2], kzs[2], oys[2], kys[2], oxs[2], kxs[2];
    auto fill = [](int par, int* off, int* k) { if (par) { off[0] = 0; k[0] = 1; return 1; } off[0] = 0; k[0] = 0; off[1] = -1; k[1] = 2; return 2; };
    const int noz = fill(pz, ozs, kzs), noy = fill(py, oys, kys), nox = fill(px, oxs, kxs);
    int nt = 0;
    for (int a = 0; a < noz; ++a)
      for (int b2 = 0; b2 < noy; ++b2)
        for (int c2 = 0; c2 < nox; ++c2)
          g.taps[nt++] = LpTap{(short)ozs[a], (short)oys[b2], (short)oxs[c2], (short)((kzs[a] * 3 + kys[b2]) * 3 + kxs[c2])};
    g.ntaps = nt; g.ooz = pz; g.ooy = py; g.oox = px;
    const int r = run();
    if (r != BTS_OK) return r;
  }
  return BTS_OK;
}

// The kernel of a call: the streaming (1x1x1), LDS-tiled (stride 2) or merged (transposed) kernel, then the gather kernels.  The partials are
// epilogues: the column sums (want_gap) leave the streaming kernel, else the gather kernel; the GroupNorm sums (G) only the merged kernel.
int lp_g_choose(const LpGCall& c, LpGChoice& ch) {
  ch = LpGChoice{};
  if (c.geo != 0 && c.geo != 2 && c.geo != 3) return BTS_ERR_UNSUPPORTED;
  if (c.geo == 0 && lp_k1_accept(c, ch)) { ch.kernel = LP_G_K1; return BTS_OK; }
  if (c.geo == 2 && lp_s2t_accept(c, ch)) { ch.kernel = LP_G_S2T; return BTS_OK; }
  if (c.geo == 3 && lp_up_accept(c, ch)) { ch.kernel = LP_G_UP; return BTS_OK; }
  if (!lp_gather_accept(c, ch)) return BTS_ERR_SHAPE;
  ch.kernel = LP_G_GATHER;
  if (!c.want_gap || ch.rows > 0) return BTS_OK;
  LpGCall plain = c;      // nobody emits the column sums: the choice of the plain call
  plain.want_gap = 0;
  return lp_g_choose(plain, ch);
}
int bts_lp_g_conv_(int dtype, LpGCall c, const LpGPtrs* ptrs, long max_rows, LpGChoice& ch, hipStream_t stream) {
  LpGPtrs q = ptrs ? *ptrs : LpGPtrs{};      // (the query's operands are aligned)
  c.x16 = lp_al16(q.x); c.wp16 = lp_al16(q.wp);
  c.y_al = lp_al16(q.y) ? 16 : ((((uintptr_t)q.y) & 7) == 0 ? 8 : 0);
  int r = lp_g_choose(c, ch);
  if (r == BTS_OK && ch.rows > max_rows) { c.want_gap = c.G = 0; r = lp_g_choose(c, ch); }
  if (!ptrs) return r;
  // (the streaming kernel with partials has only ever asked for its own conditions; every other route goes through the common check)
  if (!(r == BTS_OK && ch.kernel == LP_G_K1 && ch.rows > 0)) {
    const int chk = lp_conv_check(dtype, q.x, q.wp, q.y, c.N, c.D, c.H, c.W, c.Cin, c.ldx, c.Cout, c.ldy);
    if (chk != BTS_OK || r != BTS_OK) return chk != BTS_OK ? chk : r;
  }
  if (ch.rows == 0) q.part = nullptr;
  if (ch.kernel == LP_G_K1) return bts_lp_k1_launch_(dtype, c, ch, q, stream);
  if (ch.kernel == LP_G_S2T) return bts_lp_s2t_launch_(dtype, c, ch, q, stream);
  return ch.kernel == LP_G_UP ? bts_lp_up_launch_(dtype, c, ch, q, stream) : lp_gather_run(dtype, c, ch, q, stream);
}

// y = Conv3DTranspose(k3, s2, 'same')(x) + bias (dense fine tensor, storage type) AND the slab-mode GroupNorm statistics of y -- ConvUpsample
// (upsample.py:28-43: conv -> GroupNormalization) without the statistics pass over the fine tensor: (sum, sumsq) partials leave the
// merged transposed-conv kernel's epilogue per fine plane.  (D,H,W) = the COARSE grid.  Calls that kernel does not take, or fine z-slabs
// that are not whole planes (rows = 0), run the conv and bts_lp_gn_stats on the stored y.
extern "C" long bts_lp_convT3d_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int G) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || G <= 0 || Cout % G != 0) return -1;
  LpGChoice ch;
  bts_lp_g_conv_(0, LpGCall{3, N, D, H, W, Cin, Cin, Cout, Cout, 0, 0, G}, nullptr, LONG_MAX, ch, nullptr);
  const long fused = ch.rows > 0 ? (long)N * G * ch.rows * 16 + 64 : 0;
  const long stats = bts_lp_gn_workspace(N, 8L * D * H * W, Cout, G);
  return (fused > stats ? fused : stats) + 64;
}
extern "C" int bts_lp_convT3d_fwd_gn(int dtype, const void* x, const void* wp, const float* bias, void* y, float* mean, float* rstd,
                                     void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int G,
                                     float eps, hipStream_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || G <= 0 || Cout % G != 0) return BTS_ERR_SHAPE;
  if (workspace == nullptr || workspace_bytes < bts_lp_convT3d_fwd_gn_workspace(N, D, H, W, Cin, Cout, G) || (((uintptr_t)workspace) & 15))
    return BTS_ERR_WORKSPACE;
  const LpGPtrs q{x, wp, bias, y, reinterpret_cast<double*>(workspace)};
  LpGChoice ch;
  const int r = bts_lp_g_conv_(dtype, LpGCall{3, N, D, H, W, Cin, ldx, Cout, Cout, 0, 0, G}, &q, (workspace_bytes - 64) / (16L * N * G), ch, stream);
  if (r != BTS_OK) return r;
  const long Vf = 8L * D * H * W;
  if (ch.rows > 0) return bts_gn_finalize_partials_(q.part, mean, rstd, N * G, ch.rows, (double)(Vf * Cout / G), eps, stream);
  return bts_lp_gn_stats(dtype, y, mean, rstd, workspace, workspace_bytes, N, Vf, Cout, G, BTS_GN_SLAB, eps, stream);
}
// res = conv1x1x1(x) + bias in the storage type AND gap[n][c] = mean over the voxels of (the unrounded) res -- the block's shortcut
// and the squeeze of its gate (resnet.py:118-121) in one pass: the column sums leave the conv's epilogue as partial rows, a small
// finalize adds them.  Calls whose partial rows no kernel writes (rows = 0) run the conv and bts_lp_colsum on the stored res.
extern "C" long bts_lp_conv1_gap_workspace(int N, long V, int Cout) {
  if (N <= 0 || V <= 0 || Cout <= 0) return -1;
  const long a = ((long)N * V / 128 + 1) * Cout * 8 + 64;      // (the query cannot see Cin: an upper bound, rows of at least 128 positions)
  const long b = bts_lp_colsum_workspace(N, V, Cout);
  return a > b ? a : b;
}
extern "C" int bts_lp_conv1_gap(int dtype, const void* x, const void* wp, const float* bias, void* res, float* gap, void* workspace,
                                long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldres, hipStream_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cout <= 0) return BTS_ERR_SHAPE;
  const long V = (long)D * H * W;
  if (workspace == nullptr || workspace_bytes < bts_lp_conv1_gap_workspace(N, V, Cout) || (((uintptr_t)workspace) & 15)) return BTS_ERR_WORKSPACE;
  const LpGPtrs q{x, wp, bias, res, reinterpret_cast<double*>(workspace)};
  LpGChoice ch;
  const int r = bts_lp_g_conv_(dtype, LpGCall{0, N, D, H, W, Cin, ldx, Cout, ldres, 0, 1}, &q, workspace_bytes / (8L * N * Cout), ch, stream);
  if (r != BTS_OK) return r;
  if (ch.rows > 0) return bts_lp_colsum_finalize_(q.part, gap, N, Cout, (int)ch.rows, 1.0 / (double)V, stream);
  if (ldres != Cout) return BTS_ERR_UNSUPPORTED;
  return bts_lp_colsum(dtype, res, gap, workspace, workspace_bytes, N, V, Cout, (float)(1.0 / (double)V), stream);
}
