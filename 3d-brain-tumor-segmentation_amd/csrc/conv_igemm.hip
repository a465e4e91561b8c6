// Implicit-GEMM 3-D convolution for gfx950 on the exact-fp32 matrix pipe
// (v_mfma_f32_32x32x2_f32: bitwise a k-ordered fmaf chain, 157 TF peak = VALU peak, far easier to keep busy).
//
// One kernel serves every "gather" form the U-Net+VAE hot path needs (reference call sites:
// layers/resnet.py:30-37,80-87,96-103  layers/downsample.py:28-35  layers/upsample.py:28-33
// layers/decoder.py:55-63  layers/vae.py:92-99) and their data-gradients:
//   out[n, o*os+oo, co] (+)= act( bias[co] + sum_t sum_ci in[n, o*s + off_t, ci] * Wp[t][ci][co] )
//     K1    : 1 tap, s=1                    (1x1x1 conv, also its data-gradient with transposed Wp)
//     K3S1  : 27 taps off=t-1, s=1          (TF 'same' pad 1; data-gradient = same form, taps flipped in Wp)
//     DOWN  : 27 taps off=t,   s=2          (TF 'same' on even sizes pads (0,1); also d/dx of Conv3DTranspose)
//     UP(p) : per output-parity class p, taps {k=0:0, k=2:-1} (even) / {k=1:0} (odd), s=1, os=2, oo=p
//             (Conv3DTranspose k3 s2 'same' in gather form: every output voxel written once, no atomics;
//              also d/dx of the stride-2 conv)
//
// Data layout: activations NDHWC fp32 with an explicit pixel stride (ld) so a tensor can be a channel
// slice of a wider "level slab" (virtual concatenation, encoder.py:83-91 / decoder.py:75).
// Weights are pre-packed (bts_conv_pack) as Wp[tap][kgroup(8 ch)][half][Npad][4] so that one
// 16-byte load per lane feeds four MFMAs: lane (half h, column n) holds channels kg*8+h*4+{0..3}.
//
// Work decomposition: 256-thread workgroup = 4 waves; output tile = (32*MS*WM voxels) x (32*NS*WN couts);
// input halo tile for KGS*8 channels staged global->regs->LDS, double buffered (one barrier per stage);
// weight fragments come straight from L2/L1 (shared by the 4 waves), input fragments from LDS via
// ds_read_b128 with a 16B-odd voxel stride (S = KGS*8+4 dwords) so 16-lane groups hit distinct slots.
//
// This file: the tiled kernel, the split-K reduce kernel every splitting form finishes with, and the tiled kernel's plan (igemm_accept)
// and launch.  The engine that offers a call to the kernels is conv_engine.hip; weight packing is conv_pack.hip.
#include <stdlib.h>
#include "common.h"
#include "conv_plan.h"

#define MAXSLOT 8

struct IgemmParams {
  const float* x;
  const float* wp;
  const float* bias;
  float* y;
  int N, Di, Hi, Wi, Cin, ldx;
  int Do, Ho, Wo;  // iteration (class) grid
  int Cout, ldy, Npad, KG;
  int ODa, OHa, OWa;  // actual output tensor dims
  int os, ooz, ooy, oox;
  int s, loz, loy, lox;
  int IZ, IY, IX;
  int lgTX, lgTY, TZ;
  int ntz, nty, ntx;
  int ntaps, flags;
  int tap_sz, tap_sy, tap_sx;  // LDS dword strides of the (z,y,x) tap axes (27-tap geometries)
  int tap_lds[27];
  int tap_w[27];
  // fused second output (FUSE2): y2 = bias2 + 1x1x1 conv of the same input with wp2 (K1 packing), evaluated at the centre
  // tap of the 27-tap sweep -- the ResNet block's shortcut conv shares conv1's input tile (resnet.py:118,134)
  const float* wp2;
  const float* bias2;
  float* y2;
  int ldy2;
  // fused second INPUT (27-tap kernels, never together with FUSE2): out += 1x1x1 conv of x2 with wp2 (K1 packing), evaluated at
  // the centre tap -- the ResNet block's data gradient dx = bwd(conv1)(dc1) + bwd(shortcut)(dres) in one pass
  // (resnet.py:118,134); the x2 fragment is a 16-byte global load of the voxel's own row (no halo, no LDS)
  const float* x2;
  int ldx2;
  // split-K: blockIdx.z handles k-groups [z*kg_per, ...); raw partials go to part[z][voxel][Npad] (no bias/act)
  int ksplit, kg_per;
  float* part;
  long reserved_[3];  // (unused: keeps the kernel-argument layout, and with it the compiled kernels, as they were)
  // fused GroupNorm statistics of the output (slab semantics: group = z-slab of D/G planes, whole tiles per group):
  // every workgroup writes (sum, sum of squares) of its tile to gnp[((n*G+g)*gn_B + b)*2], b = tile index inside the group
  double* gnp;
  int gn_G, gn_zt;  // groups; z-tiles per group
  int gn_gridy;     // host side: grid.y of the launch (partials per group = gn_zt*nty*ntx*gn_gridy)
  // merged launch of the 8 output-parity classes of the UP geometry (blockIdx.z = class)
  int ncls;
  int cls_nt[8];
  int cls_tl[8][8];
  int cls_tw[8][8];
};

// One stage of the implicit GEMM: nkg k-groups (8 input channels each) x NT taps, fully unrolled over the taps.
template <int NT, int MS, int NS, bool F2 = false, bool FIXG = false>
__device__ __forceinline__ void stage_taps(const IgemmParams& p, const int* tlp, const int* twp, const float* cur,
                                           const int (&bbase)[MS], const int (&lane_woff)[NS], int kg0, int nkg,
                                           f32x16 (&acc)[MS][NS], f32x16 (*acc2)[NS], const float* const (&x2row)[MS],
                                           bool have_x2) {
  const int wstepKG = 2 * p.Npad * 4;       // floats between consecutive k-groups of one tap
  const int wstepTap = p.KG * wstepKG;      // floats between consecutive taps
  // 27-tap geometries (k3s1, DOWN): LDS offset and weight tap index are arithmetic in the compile-time tap number, so
  // nothing is loaded inside the tap sequence (an s_load there shares lgkmcnt with the ds_read prefetch and drains it);
  // the UP parity classes (<= 8 taps) keep their small tables in SGPRs.
  int tl[NT], tw[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (NT == 27) {
      // FIXG: the 32x4xTZ tile of the big-grid configs has a compile-time halo geometry (IX=34, IY=6, S=12), so every
      // tap offset folds into the ds_read immediate: no per-tap address VALU, no address registers
      tl[t] = FIXG ? (((t / 9) * 6 + (t / 3) % 3) * 34 + (t % 3)) * 12
                   : (t / 9) * p.tap_sz + ((t / 3) % 3) * p.tap_sy + (t % 3) * p.tap_sx;
      tw[t] = t * wstepTap;
    } else {
      tl[t] = tlp[t];
      tw[t] = twp[t] * wstepTap;
    }
  }
  for (int kgl = 0; kgl < nkg; ++kgl) {
    const int wk = (kg0 + kgl) * wstepKG;
    const float* lb = cur + kgl * 8;
    // prefetch depths: weights (L2, ~500-900 cycles) AD taps ahead, input fragments (LDS, ~130 cycles) BD taps ahead;
    // deep enough that a single wave per SIMD keeps the matrix pipe fed while its partner workgroup is in its prologue
    constexpr int AD = 2, BD = 1;  // deeper (3/2) measured neutral on MI355X and costs registers
    f32x4 a[AD + 1][NS], b[BD + 1][MS];
    f32x4 a2s[NS];
    f32x4 b2in[MS];
    const bool fin = (NT == 27) && !F2 && have_x2;
    if (fin) {  // second input: this voxel's 8 channels of the k-group, requested a whole stage ahead of their use
#pragma unroll
      for (int ms = 0; ms < MS; ++ms) b2in[ms] = *reinterpret_cast<const f32x4*>(x2row[ms] + (kg0 + kgl) * 8);
    }
#pragma unroll
    for (int q = 0; q < AD; ++q)
      if (q < NT) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
          a[q][ns] = *reinterpret_cast<const f32x4*>((p.wp + (wk + tw[q < NT ? q : 0])) + lane_woff[ns]);
      }
#pragma unroll
    for (int q = 0; q < BD; ++q)
      if (q < NT) {
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) b[q][ms] = *reinterpret_cast<const f32x4*>(lb + bbase[ms] + tl[q < NT ? q : 0]);
      }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t + AD < NT) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
          a[(t + AD) % (AD + 1)][ns] =
              *reinterpret_cast<const f32x4*>((p.wp + (wk + tw[t + AD < NT ? t + AD : 0])) + lane_woff[ns]);  // scalar base + lane offset
      }
      if (t + BD < NT) {
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
          b[(t + BD) % (BD + 1)][ms] = *reinterpret_cast<const f32x4*>(lb + bbase[ms] + tl[t + BD < NT ? t + BD : 0]);
      }
      if (F2 && NT == 27 && t == 11) {  // shortcut-conv weights, two taps ahead of the centre tap
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) a2s[ns] = *reinterpret_cast<const f32x4*>((p.wp2 + wk) + lane_woff[ns]);
      }
      if (!F2 && NT == 27 && t == 11) {
        if (fin) {
#pragma unroll
          for (int ns = 0; ns < NS; ++ns) a2s[ns] = *reinterpret_cast<const f32x4*>((p.wp2 + wk) + lane_woff[ns]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // prefetches are issued before this tap's MFMAs, not sunk behind them
      if (F2 && NT == 27 && t == 13) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int ns = 0; ns < NS; ++ns)
              acc2[ms][ns] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2s[ns][j], b[t % (BD + 1)][ms][j], acc2[ms][ns], 0, 0, 0);
      }
      if (!F2 && NT == 27 && t == 13) {
        if (fin) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ms = 0; ms < MS; ++ms)
#pragma unroll
              for (int ns = 0; ns < NS; ++ns)
                acc[ms][ns] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2s[ns][j], b2in[ms][j], acc[ms][ns], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
          for (int ns = 0; ns < NS; ++ns)
            acc[ms][ns] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t % (AD + 1)][ns][j], b[t % (BD + 1)][ms][j], acc[ms][ns], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);  // keep the hand-written 2-deep pipeline: no hoisting of later taps' loads
    }
  }
}

// TRI: three resident workgroups per CU instead of two (single-buffered halo tile, <= 168 VGPRs): whenever one
// workgroup is in its prologue / refill / epilogue the SIMD still holds two MFMA-issuing waves.
#define IG_TRI(MS, NS, KGS, FUSE2, FIXG) ((MS) == 2 && (NS) == 1 && (KGS) == 1 && !(FUSE2) && (FIXG))
template <int MS, int NS, int WM, int WN, int KGS, bool FUSE2 = false, bool FIXG = false, bool T27 = false>
__global__ __launch_bounds__(256, IG_TRI(MS, NS, KGS, FUSE2, FIXG) ? 3 : 2) void igemm_kernel(const IgemmParams p) {
  constexpr bool SINGLE = IG_TRI(MS, NS, KGS, FUSE2, FIXG);
  constexpr int S = KGS * 8 + 4;  // dwords per staged voxel (pad 4: 16B-odd stride)
  constexpr int QPV = KGS * 2;    // float4 slots per voxel
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int h = lane >> 5, l32 = lane & 31;

  int b = blockIdx.x;
  const int tx = b % p.ntx; b /= p.ntx;
  const int ty = b % p.nty; b /= p.nty;
  const int tz = b % p.ntz;
  const int n = b / p.ntz;
  const int TX = 1 << p.lgTX, TY = 1 << p.lgTY;
  int ntaps = p.ntaps, ooz = p.ooz, ooy = p.ooy, oox = p.oox;
  const int* tlp = p.tap_lds;
  const int* twp = p.tap_w;
  if (p.ncls > 1) {
    const int cls = blockIdx.z;
    ntaps = p.cls_nt[cls]; tlp = p.cls_tl[cls]; twp = p.cls_tw[cls];
    ooz = (cls >> 2) & 1; ooy = (cls >> 1) & 1; oox = cls & 1;
  }
  const int oz0 = tz * p.TZ, oy0 = ty * TY, ox0 = tx * TX;
  const int iz0 = oz0 * p.s + p.loz, iy0 = oy0 * p.s + p.loy, ix0 = ox0 * p.s + p.lox;
  const int tileVox = p.IZ * p.IY * p.IX;
  const int bufDw = tileVox * S;

  // ---- staging map: slot e = tid + i*256 -> (voxel, quad). Only a 32-bit element offset relative to the tile origin
  //      is kept per slot (-1 = zero padding); LDS offset and channel quad are recomputed from e (QPV is a constant).
  const int nslots = tileVox * QPV;
  const float* xbase = p.x + ((((long)n * p.Di + iz0) * p.Hi + iy0) * p.Wi + ix0) * (long)p.ldx;  // wave-uniform
  int goff[MAXSLOT];
  const int IYX = p.IY * p.IX;
  const float invIX = 1.0f / (float)p.IX, invIYX = 1.0f / (float)IYX;
#pragma unroll
  for (int i = 0; i < MAXSLOT; ++i) {
    const int e = tid + i * 256;
    goff[i] = -1;
    if (e < nslots) {
      const int vox = e / QPV, q = e - vox * QPV;
      // exact small-integer division by float reciprocal (operands < 2^16): the prologue is on every workgroup's
      // critical path, integer division would cost ~50 VALU instructions per slot
      const int vz = (int)(((float)vox + 0.5f) * invIYX);
      const int r = vox - vz * IYX;
      const int vy = (int)(((float)r + 0.5f) * invIX);
      const int vx = r - vy * p.IX;
      if ((unsigned)(iz0 + vz) < (unsigned)p.Di && (unsigned)(iy0 + vy) < (unsigned)p.Hi && (unsigned)(ix0 + vx) < (unsigned)p.Wi)
        goff[i] = ((vz * p.Hi + vy) * p.Wi + vx) * p.ldx + q * 4;
    }
  }

  // ---- fragment bases ----
  int bbase[MS];
#pragma unroll
  for (int ms = 0; ms < MS; ++ms) {
    const int m = (wm * MS + ms) * 32 + l32;
    const int mx = m & (TX - 1);
    const int my = (m >> p.lgTX) & (TY - 1);
    const int mz = m >> (p.lgTX + p.lgTY);
    bbase[ms] = ((mz * p.s * p.IY + my * p.s) * p.IX + mx * p.s) * S + h * 4;
  }
  int lane_woff[NS];  // float offset of this lane's weight quad inside one (tap, k-group) image
#pragma unroll
  for (int ns = 0; ns < NS; ++ns) {
    int ncol = ((blockIdx.y * WN + wn) * NS + ns) * 32 + l32;
    if (ncol >= p.Npad) ncol = p.Npad - 1;  // tile wider than the padded cout range: results are discarded
    lane_woff[ns] = (h * p.Npad + ncol) * 4;
  }

  const float* x2row[MS];
#pragma unroll
  for (int ms = 0; ms < MS; ++ms) {
    x2row[ms] = nullptr;
    if (p.x2) {
      const int m = (wm * MS + ms) * 32 + l32;
      int oz = oz0 + (m >> (p.lgTX + p.lgTY)), oy = oy0 + ((m >> p.lgTX) & (TY - 1)), ox = ox0 + (m & (TX - 1));
      if (oz >= p.Do) oz = p.Do - 1;   // voxels past the edge are computed and discarded: keep their loads in bounds
      if (oy >= p.Ho) oy = p.Ho - 1;
      if (ox >= p.Wo) ox = p.Wo - 1;
      x2row[ms] = p.x2 + ((((long)n * p.Do + oz) * p.Ho + oy) * p.Wo + ox) * (long)p.ldx2 + h * 4;
    }
  }
  const bool have_x2 = p.x2 != nullptr;
  f32x16 acc[MS][NS];
#pragma unroll
  for (int ms = 0; ms < MS; ++ms)
#pragma unroll
    for (int ns = 0; ns < NS; ++ns)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ms][ns][r] = 0.f;
  f32x16 acc2[FUSE2 ? MS : 1][NS];
  if (FUSE2) {
#pragma unroll
    for (int ms = 0; ms < MS; ++ms)
#pragma unroll
      for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[ms][ns][r] = 0.f;
  }

  int kgBeg = 0, kgEnd = p.KG;
  if (p.ksplit > 1) {
    kgBeg = blockIdx.z * p.kg_per;
    kgEnd = kgBeg + p.kg_per;
    if (kgEnd > p.KG) kgEnd = p.KG;
  }
  const int stBeg = kgBeg / KGS;  // kg_per is a multiple of KGS
  const int nstages = (kgEnd - kgBeg + KGS - 1) / KGS;
  const bool vecin = (p.flags & IG_FLAG_VECIN) != 0;

  f32x4 pre[MAXSLOT];
  auto fetch = [&](int st) {
    const int c0 = (stBeg + st) * KGS * 8;
#pragma unroll
    for (int i = 0; i < MAXSLOT; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (goff[i] >= 0) {
        const int c = c0 + ((tid + i * 256) % QPV) * 4;
        const float* src = xbase + goff[i] + c0;
        if (vecin) {
          if (c < p.Cin) v = *reinterpret_cast<const f32x4*>(src);
        } else {
          if (c + 0 < p.Cin) v[0] = src[0];
          if (c + 1 < p.Cin) v[1] = src[1];
          if (c + 2 < p.Cin) v[2] = src[2];
          if (c + 3 < p.Cin) v[3] = src[3];
        }
      }
      pre[i] = v;
    }
  };
  auto commit = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < MAXSLOT; ++i) {
      const int e = tid + i * 256;
      if (e < nslots) *reinterpret_cast<f32x4*>(buf + (e / QPV) * S + (e % QPV) * 4) = pre[i];
    }
  };

  fetch(0);
  commit(lds);
  __syncthreads();

  for (int st = 0; st < nstages; ++st) {
    const float* cur = SINGLE ? lds : lds + (st & 1) * bufDw;
    float* nxt = SINGLE ? lds : lds + ((st + 1) & 1) * bufDw;
    const bool more = (st + 1) < nstages;
    if (more) fetch(st + 1);

    // k-groups of this stage x taps: fully unrolled tap sequence (tables hoisted to SGPRs), weight fragments
    // prefetched two taps ahead and input fragments one tap ahead so their latencies sit under the MFMAs
    const int kg0 = (stBeg + st) * KGS;
    int nkg = kgEnd - kg0;
    if (nkg > KGS) nkg = KGS;
    if constexpr (FIXG || T27 || FUSE2) {  // 27-tap form known at compile time (fixed geometry, the fused pair, or
      // the launcher's T27 instantiation for k3s1 / stride-2 convs): no runtime tap-count dispatch, so the accumulators
      // are not shuffled between register sets around a switch
      stage_taps<27, MS, NS, FUSE2, FIXG>(p, tlp, twp, cur, bbase, lane_woff, kg0, nkg, acc, acc2, x2row, have_x2);
    } else if constexpr (KGS == 1) {
      switch (ntaps) {
        case 27: stage_taps<27, MS, NS, FUSE2, FIXG>(p, tlp, twp, cur, bbase, lane_woff, kg0, nkg, acc, acc2, x2row, have_x2); break;
        case 8: stage_taps<8, MS, NS>(p, tlp, twp, cur, bbase, lane_woff, kg0, nkg, acc, nullptr, x2row, false); break;
        case 4: stage_taps<4, MS, NS>(p, tlp, twp, cur, bbase, lane_woff, kg0, nkg, acc, nullptr, x2row, false); break;
        case 2: stage_taps<2, MS, NS>(p, tlp, twp, cur, bbase, lane_woff, kg0, nkg, acc, nullptr, x2row, false); break;
        default: stage_taps<1, MS, NS>(p, tlp, twp, cur, bbase, lane_woff, kg0, nkg, acc, nullptr, x2row, false); break;
      }
    } else {  // the 4-k-group staging variant only serves the 1x1x1 convolutions
      stage_taps<1, MS, NS>(p, tlp, twp, cur, bbase, lane_woff, kg0, nkg, acc, nullptr, x2row, false);
    }
    if (SINGLE) __syncthreads();  // every wave has finished reading the tile before it is overwritten
    if (more) commit(nxt);
    __syncthreads();
  }

  // ---- split-K: raw partial tile to the workspace, finished by igemm_reduce_kernel ----
  if (p.ksplit > 1) {
    const long nvox = (long)p.N * p.Do * p.Ho * p.Wo;
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) {
      const int m = (wm * MS + ms) * 32 + l32;
      const int oz = oz0 + (m >> (p.lgTX + p.lgTY)), oy = oy0 + ((m >> p.lgTX) & (TY - 1)), ox = ox0 + (m & (TX - 1));
      if (oz >= p.Do || oy >= p.Ho || ox >= p.Wo) continue;
      const long v = (((long)n * p.Do + oz) * p.Ho + oy) * p.Wo + ox;
      float* row = p.part + ((long)blockIdx.z * nvox + v) * p.Npad;
#pragma unroll
      for (int ns = 0; ns < NS; ++ns) {
        const int nb = ((blockIdx.y * WN + wn) * NS + ns) * 32;
        if (nb >= p.Npad) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v4 = {acc[ms][ns][4 * g + 0], acc[ms][ns][4 * g + 1], acc[ms][ns][4 * g + 2], acc[ms][ns][4 * g + 3]};
          *reinterpret_cast<f32x4*>(row + nb + 8 * g + 4 * h) = v4;
        }
      }
    }
    return;
  }

  // ---- epilogue: D rows = couts (4 consecutive per register quad), cols = voxels ----
  const bool vecout = (p.flags & IG_FLAG_VECOUT) != 0;
  float gn_s = 0.f, gn_q = 0.f;  // this lane's share of the tile's GroupNorm sums (<= 64 values)
#pragma unroll
  for (int ms = 0; ms < MS; ++ms) {
    const int m = (wm * MS + ms) * 32 + l32;
    const int mx = m & (TX - 1);
    const int my = (m >> p.lgTX) & (TY - 1);
    const int mz = m >> (p.lgTX + p.lgTY);
    const int oz = oz0 + mz, oy = oy0 + my, ox = ox0 + mx;
    if (oz >= p.Do || oy >= p.Ho || ox >= p.Wo) continue;
    const long pix = (((long)n * p.ODa + (oz * p.os + ooz)) * p.OHa + (oy * p.os + ooy)) * p.OWa + (ox * p.os + oox);
    float* yrow = p.y + pix * p.ldy;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      const int nb = ((blockIdx.y * WN + wn) * NS + ns) * 32;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co = nb + 8 * g + 4 * h;
        if (co >= p.Cout) continue;
        f32x4 v = {acc[ms][ns][4 * g + 0], acc[ms][ns][4 * g + 1], acc[ms][ns][4 * g + 2], acc[ms][ns][4 * g + 3]};
        if (p.flags & IG_FLAG_BIAS) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co + j < p.Cout) v[j] += p.bias[co + j];
        }
        if (p.gnp) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co + j < p.Cout) { gn_s += v[j]; gn_q = fmaf(v[j], v[j], gn_q); }
        }
        if (p.flags & IG_FLAG_SIGMOID) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = sigmoidf_(v[j]);
        }
        if (vecout) {
          f32x4* dst = reinterpret_cast<f32x4*>(yrow + co);
          if (p.flags & IG_FLAG_ACCUM) {
            f32x4 o = *dst;
            v += o;
          }
          *dst = v;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co + j < p.Cout) {
              float r = v[j];
              if (p.flags & IG_FLAG_ACCUM) r += yrow[co + j];
              yrow[co + j] = r;
            }
        }
        if (FUSE2) {  // shortcut output: bias only, dense or strided rows, same cout tiling
          float* y2row = p.y2 + pix * p.ldy2;
          f32x4 v2 = {acc2[FUSE2 ? ms : 0][ns][4 * g + 0], acc2[FUSE2 ? ms : 0][ns][4 * g + 1],
                      acc2[FUSE2 ? ms : 0][ns][4 * g + 2], acc2[FUSE2 ? ms : 0][ns][4 * g + 3]};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (p.bias2 && co + j < p.Cout) v2[j] += p.bias2[co + j];
          if (vecout && (p.ldy2 % 4 == 0)) *reinterpret_cast<f32x4*>(y2row + co) = v2;
          else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (co + j < p.Cout) y2row[co + j] = v2[j];
          }
        }
      }
    }
  }
  if (p.gnp) {  // fixed-order combine: lanes (shuffle tree) -> 4 waves (LDS) -> one (sum, sumsq) pair per workgroup
    double ds = wave_sum_f64((double)gn_s), dq = wave_sum_f64((double)gn_q);
    double* sh = reinterpret_cast<double*>(lds);  // the staging buffers are idle (last barrier passed)
    if (lane == 0) { sh[wave * 2] = ds; sh[wave * 2 + 1] = dq; }
    __syncthreads();
    if (tid == 0) {
      const int g = tz / p.gn_zt;
      const long B = (long)p.gn_zt * p.nty * p.ntx * gridDim.y;
      const long b_ = (((long)(tz - g * p.gn_zt) * p.nty + ty) * p.ntx + tx) * gridDim.y + blockIdx.y;
      double* o = p.gnp + (((long)n * p.gn_G + g) * B + b_) * 2;
      o[0] = sh[0] + sh[2] + sh[4] + sh[6];
      o[1] = sh[1] + sh[3] + sh[5] + sh[7];
    }
  }
}

// split-K finish: y[v][co] (+)= act(bias[co] + sum_z part[z][v][co]); fixed summation order (deterministic)
__global__ __launch_bounds__(256) void igemm_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                           float* __restrict__ y, long nvox, int Cout, int Npad, int ldy,
                                                           int ksplit, int flags) {
  const long total = nvox * Cout;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long v = i / Cout;
    const int co = (int)(i - v * Cout);
    float s = 0.f;
    for (int z = 0; z < ksplit; ++z) s += part[((long)z * nvox + v) * Npad + co];
    if (flags & IG_FLAG_BIAS) s += bias[co];
    if (flags & IG_FLAG_SIGMOID) s = sigmoidf_(s);
    float* d = y + v * ldy + co;
    *d = (flags & IG_FLAG_ACCUM) ? *d + s : s;
  }
}

int bts_igemm_reduce_(const float* part, const float* bias, float* y, long nvox, int Cout, int Npad, int ldy, int ksplit, int flags,
                      hipStream_t stream) {
  long blocks = (nvox * Cout + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  (void)hipGetLastError();
  hipLaunchKernelGGL(igemm_reduce_kernel, dim3((int)blocks), dim3(256), 0, stream, part, bias, y, nvox, Cout, Npad, ldy, ksplit, flags);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Launch logic
// ---------------------------------------------------------------------------------------------

// cfg ids: IgemmPlan (conv_plan.h)
static int choose_cfg(int geo, int N, int Do, int Ho, int Wo, int Npad, int* Mout) {
  const long vox = (long)Do * Ho * Wo;
  int M, cfg;
  if (geo == GEO_DOWN) {
    M = 64;
    cfg = (Npad >= 128) ? 2 : 3;
  } else {
    const long wg256 = (long)N * ((vox + 255) / 256) * ((Npad + 63) / 64);
    if (Npad <= 32) {
      if ((long)N * ((vox + 255) / 256) >= 512) { M = 256; cfg = 0; }
      else { M = 128; cfg = 4; }
    } else if (wg256 >= 512) { M = 256; cfg = 1; }
    else {
      M = 64;
      const long wg64_128 = (long)N * ((vox + 63) / 64) * ((Npad + 127) / 128);
      cfg = (Npad >= 128 && wg64_128 >= 384) ? 2 : 3;
    }
  }
  *Mout = M;
  return cfg;
}

// The tiled kernel takes every call of the family, so this one returns a status: BTS_OK with the plan (config, tile geometry, split-K,
// GroupNorm slots), BTS_ERR_UNSUPPORTED for the fused shortcut output on cfg 1 (the 64-accumulator tiling has no registers for the
// second set), BTS_ERR_SHAPE for a halo tile beyond the staging slots.
int igemm_accept(const ConvCall& c, ConvChoice& ch) {
  IgemmPlan& g = ch.g;
  const bool k1 = c.geo == GEO_K1, up = c.geo == GEO_UP, fuse2 = c.second == CONV_Y2;
  const int Do = up ? c.Di : c.Do, Ho = up ? c.Hi : c.Ho, Wo = up ? c.Wi : c.Wo;      // the iteration grid (UP: one parity class)
  const int Npad = conv_npad32(c.Cout), KG = (c.Cin + 7) / 8, KGS = k1 ? 4 : 1;
  int M;  // voxels per workgroup tile
  g.cfg = choose_cfg(c.geo, up ? 8 * c.N : c.N, Do, Ho, Wo, Npad, &M);
  if (fuse2 && g.cfg == 1) return BTS_ERR_UNSUPPORTED;
  // tile dims (powers of two in x,y)
  int TX = 32;
  while (TX > 4 && TX / 2 >= Wo) TX /= 2;  // smallest pow2 >= Wo, capped at 32
  if (c.geo == GEO_DOWN && TX > 8) TX = 8;
  if (TX > M) TX = M;
  int TY = 4;
  while (TY > 1 && TY / 2 >= Ho) TY /= 2;
  if (TX * TY > M) TY = M / TX;
  int TZ = M / (TX * TY);
  // prefer shrinking z extent into y when the volume is shallow in z
  while (TZ > 1 && TZ / 2 >= Do && TY * 2 <= 64) { TZ /= 2; TY *= 2; }
  g.lgTX = ilog2(TX); g.lgTY = ilog2(TY); g.TZ = TZ;
  g.ntx = (Wo + TX - 1) / TX; g.nty = (Ho + TY - 1) / TY; g.ntz = (Do + TZ - 1) / TZ;
  const int s = c.geo == GEO_DOWN ? 2 : 1, span = k1 ? 1 : up ? 2 : 3;      // input stride; taps per axis
  g.IX = (TX - 1) * s + span; g.IY = (TY - 1) * s + span; g.IZ = (TZ - 1) * s + span;
  if (g.IZ * g.IY * g.IX * KGS * 2 > 256 * MAXSLOT) return BTS_ERR_SHAPE;
  static const int NT[5] = {32, 64, 128, 64, 32};      // couts per workgroup of the config
  g.gridy = (Npad + NT[g.cfg] - 1) / NT[g.cfg];
  // split-K when the tile grid cannot fill the chip and the contraction is long (tiny spatial grids, wide channels)
  g.ksplit = 1;
  g.kg_per = KG;
  g.need = 0;
  const long wgs = (long)((unsigned)c.N * g.ntz * g.nty * g.ntx) * g.gridy;
  // two workgroups fit a CU: below 512 tiles the chip is not full and a single wave per SIMD cannot keep the matrix
  // pipe busy, so the contraction is split (measured: 16^3 256->256 0.157 -> 0.137 ms, 16^3 768->256 0.46 -> 0.38 ms);
  // the 1x1x1 staging variant has too little work per k-group for that and keeps the old, lower threshold
  const long sk_below = k1 ? 192 : 512, sk_target = k1 ? 384 : 512;
  if (!fuse2 && !up && wgs < sk_below && KG >= 4 * KGS) {
    int ks = (int)((sk_target + wgs - 1) / wgs);
    const int maxks = KG / (2 * KGS);
    if (ks > maxks) ks = maxks;
    if (ks > 64) ks = 64;
    if (ks > 1) {
      int per = (KG + ks - 1) / ks;
      per = (per + KGS - 1) / KGS * KGS;
      ks = (KG + per - 1) / per;
      const long need = (long)ks * c.N * Do * Ho * Wo * Npad * 4;
      if (ks > 1 && c.ws_bytes >= need) {
        g.ksplit = ks;
        g.kg_per = per;
        g.need = need;
      }
    }
  }
  // split-K tiles are finished by the reduce kernel: no fused statistics; nor from the parity classes
  g.gn_zt = (g.ksplit > 1 || up) ? 0 : conv_gn_zt(c, TZ);
  ch.sym = g.cfg + (k1 ? SYM_IGEMM_K1 : 0);
  ch.ws = g.need;
  ch.gn_B = (long)g.gn_zt * g.nty * g.ntx * g.gridy;
  return BTS_OK;
}

template <int MS, int NS, int WM, int WN, int KGS, bool FUSE2 = false, bool FIXG = false, bool T27 = false>
static int launch_cfg(const IgemmParams& p, const ConvChoice& ch, hipStream_t stream) {
  constexpr int S = KGS * 8 + 4;
  const int tileVox = p.IZ * p.IY * p.IX;
  // a single stage (all channels fit one staging pass, e.g. the 1x1x1 convs with Cin <= 32) needs no second buffer:
  // half the LDS -> twice the resident workgroups to hide the (then un-overlapped) staging latency
  const int nstages_all = (p.KG + KGS - 1) / KGS;
  const size_t shmem = (size_t)((nstages_all > 1 && !IG_TRI(MS, NS, KGS, FUSE2, FIXG)) ? 2 : 1) * tileVox * S * sizeof(float);
  auto kern = igemm_kernel<MS, NS, WM, WN, KGS, FUSE2, FIXG, T27>;
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  const dim3 grid(p.N * p.ntz * p.nty * p.ntx, ch.g.gridy, p.ncls > 1 ? p.ncls : p.ksplit);
  const bool prof = bts_prof_on();
  if (prof) {
    const double taps = (p.ncls > 1) ? 27.0 : (double)p.ntaps;
    bts_prof_begin(ch.sym, 2.0 * taps * p.Cin * p.Cout * (double)p.N * p.Do * p.Ho * p.Wo, stream);
  }
  (void)hipGetLastError(); hipLaunchKernelGGL(kern, grid, dim3(256), shmem, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  if (p.ksplit <= 1) return BTS_OK;
  return bts_igemm_reduce_(p.part, p.bias, p.y, (long)p.N * p.Do * p.Ho * p.Wo, p.Cout, p.Npad, p.ldy, p.ksplit, p.flags, stream);
}

// The launch igemm_accept planned: the tap tables of the geometry (UP: one per parity class) on the plan's tiles, and the instantiation
// of its config.
int bts_igemm_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
  const IgemmPlan& g = ch.g;
  const bool k1 = c.geo == GEO_K1, up = c.geo == GEO_UP;
  IgemmParams p;
  p.wp2 = c.second ? q.wp2 : nullptr;
  p.bias2 = c.second == CONV_Y2 ? q.bias2 : nullptr; p.y2 = c.second == CONV_Y2 ? q.y2 : nullptr; p.ldy2 = c.second == CONV_Y2 ? c.ld2 : 0;
  p.x2 = c.second == CONV_X2 ? q.x2 : nullptr; p.ldx2 = c.second == CONV_X2 ? c.ld2 : 0;   // second input (x2 + wp2 without y2): see IgemmParams
  p.part = reinterpret_cast<float*>(q.ws);
  p.x = q.x; p.wp = q.wp; p.bias = q.bias; p.y = q.y;
  p.N = c.N; p.Di = c.Di; p.Hi = c.Hi; p.Wi = c.Wi; p.Cin = c.Cin; p.ldx = c.ldx;
  p.Do = up ? c.Di : c.Do; p.Ho = up ? c.Hi : c.Ho; p.Wo = up ? c.Wi : c.Wo; p.Cout = c.Cout; p.ldy = c.ldy;
  p.Npad = conv_npad32(c.Cout); p.KG = (c.Cin + 7) / 8;
  p.ODa = c.Do; p.OHa = c.Ho; p.OWa = c.Wo;
  p.os = up ? 2 : 1; p.ooz = p.ooy = p.oox = 0;
  p.s = c.geo == GEO_DOWN ? 2 : 1;
  p.flags = c.flags;
  if ((c.ldx % 4 == 0) && (c.Cin % 4 == 0) && c.x16) p.flags |= IG_FLAG_VECIN;
  if ((c.ldy % 4 == 0) && (c.Cout % 4 == 0) && c.y16) p.flags |= IG_FLAG_VECOUT;
  p.lgTX = g.lgTX; p.lgTY = g.lgTY; p.TZ = g.TZ; p.ntx = g.ntx; p.nty = g.nty; p.ntz = g.ntz; p.IX = g.IX; p.IY = g.IY; p.IZ = g.IZ;
  p.ksplit = g.ksplit; p.kg_per = g.kg_per;
  p.gnp = g.gn_zt ? q.gnp : nullptr; p.gn_G = g.gn_zt ? c.G : 0; p.gn_zt = g.gn_zt ? g.gn_zt : 1; p.gn_gridy = g.gridy;

  // tap table: offsets relative to o*s, LDS offsets relative to the tile's low corner
  const int lo = (c.geo == GEO_S1 || up) ? -1 : 0;      // (UP: the common halo of the 8 classes, offset -1 on every axis)
  const int S = (k1 ? 4 : 1) * 8 + 4;
  p.ntaps = k1 ? 1 : up ? 8 : 27;      // (UP: placeholder; the per-class tables are below)
  p.ncls = 1;
  p.loz = p.loy = p.lox = lo;
  for (int t = 0; t < 27; ++t) {
    p.tap_lds[t] = (k1 || up || t >= p.ntaps) ? 0 : ((t / 9 * p.IY + (t / 3) % 3) * p.IX + t % 3) * S;      // (S1: t - 1 - lo = DOWN: t - lo)
    p.tap_w[t] = (k1 || up) ? 0 : t;
  }
  p.tap_sz = p.IY * p.IX * S; p.tap_sy = p.IX * S; p.tap_sx = S;
  if (up) {
    p.ncls = 8;
    for (int cl = 0; cl < 8; ++cl) {
      const int par[3] = {(cl >> 2) & 1, (cl >> 1) & 1, cl & 1};
      int k[3][2], d[3][2], n[3];
      for (int a = 0; a < 3; ++a) {
        if (par[a] == 0) { k[a][0] = 0; d[a][0] = 0; k[a][1] = 2; d[a][1] = -1; n[a] = 2; }
        else { k[a][0] = 1; d[a][0] = 0; n[a] = 1; }
      }
      int ct = 0;
      for (int a = 0; a < n[0]; ++a)
        for (int bb = 0; bb < n[1]; ++bb)
          for (int cc = 0; cc < n[2]; ++cc) {
            p.cls_tl[cl][ct] = (((d[0][a] + 1) * p.IY + (d[1][bb] + 1)) * p.IX + (d[2][cc] + 1)) * S;
            p.cls_tw[cl][ct] = (k[0][a] * 3 + k[1][bb]) * 3 + k[2][cc];
            ++ct;
          }
      p.cls_nt[cl] = ct;
      for (; ct < 8; ++ct) { p.cls_tl[cl][ct] = 0; p.cls_tw[cl][ct] = 0; }
    }
  }

  const bool fixg = (c.geo == GEO_S1) && p.IX == 34 && p.IY == 6;
  if (fixg && (g.cfg == 0 || g.cfg == 1)) {
    if (p.y2 != nullptr) return launch_cfg<2, 1, 4, 1, 1, true, true>(p, ch, stream);      // (cfg 0: igemm_accept refused cfg 1)
    if (g.cfg == 0) return launch_cfg<2, 1, 4, 1, 1, false, true>(p, ch, stream);
    return launch_cfg<2, 2, 4, 1, 1, false, true>(p, ch, stream);
  }
  if (k1) {
    switch (g.cfg) {
      case 0: return launch_cfg<2, 1, 4, 1, 4>(p, ch, stream);
      case 1: return launch_cfg<2, 2, 4, 1, 4>(p, ch, stream);
      case 2: return launch_cfg<1, 2, 2, 2, 4>(p, ch, stream);
      case 3: return launch_cfg<1, 1, 2, 2, 4>(p, ch, stream);
      default: return launch_cfg<1, 1, 4, 1, 4>(p, ch, stream);
    }
  }
  if (p.y2 != nullptr) {  // fused shortcut conv: every tiling but the 64-accumulator one has the registers
    switch (g.cfg) {
      case 0: return launch_cfg<2, 1, 4, 1, 1, true>(p, ch, stream);
      case 2: return launch_cfg<1, 2, 2, 2, 1, true>(p, ch, stream);
      case 3: return launch_cfg<1, 1, 2, 2, 1, true>(p, ch, stream);
      default: return launch_cfg<1, 1, 4, 1, 1, true>(p, ch, stream);
    }
  }
  if (!up) {      // 27 taps, one class
    switch (g.cfg) {
      case 0: return launch_cfg<2, 1, 4, 1, 1, false, false, true>(p, ch, stream);
      case 1: return launch_cfg<2, 2, 4, 1, 1, false, false, true>(p, ch, stream);
      case 2: return launch_cfg<1, 2, 2, 2, 1, false, false, true>(p, ch, stream);
      case 3: return launch_cfg<1, 1, 2, 2, 1, false, false, true>(p, ch, stream);
      default: return launch_cfg<1, 1, 4, 1, 1, false, false, true>(p, ch, stream);
    }
  }
  switch (g.cfg) {
    case 0: return launch_cfg<2, 1, 4, 1, 1>(p, ch, stream);
    case 1: return launch_cfg<2, 2, 4, 1, 1>(p, ch, stream);
    case 2: return launch_cfg<1, 2, 2, 2, 1>(p, ch, stream);
    case 3: return launch_cfg<1, 1, 2, 2, 1>(p, ch, stream);
    default: return launch_cfg<1, 1, 4, 1, 1>(p, ch, stream);
  }
}
