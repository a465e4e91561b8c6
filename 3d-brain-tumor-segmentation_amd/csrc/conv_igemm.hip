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
// Also in this translation unit (they share the packed-weight layout, the flag bits and the split-K reduce kernel):
//   upm_kernel  -- UP form with all 8 output-parity classes per workgroup (Conv3DTranspose forward, stride-2 data gradient)
//   k1s_kernel  -- LDS-free streaming 1x1x1 conv for big grids
//   dsc_kernel  -- vector-ALU direct 3x3x3 conv for <= 4 output channels
//   c2_kernel   -- 3x3x3 conv of a 2-channel input (the MFMA's K = 2 is the channel pair)
// The K3S1 weight image carries a second, Winograd-domain part; stride-1 3x3x3 launches are offered to conv_wino.hip first.
// and the fused entry points: shortcut pair (FUSE2), GroupNorm statistics in the epilogue, data-gradient pair (second input).
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

int bts_igemm_reduce_(const float* part, const float* bias, float* y, long nvox, int Cout, int Npad, int ldy, int ksplit,
                      int with_bias, int accum, hipStream_t stream) {
  long blocks = (nvox * Cout + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  (void)hipGetLastError();
  hipLaunchKernelGGL(igemm_reduce_kernel, dim3((int)blocks), dim3(256), 0, stream, part, bias, y, nvox, Cout, Npad, ldy, ksplit,
                     (with_bias ? IG_FLAG_BIAS : 0) | (accum ? IG_FLAG_ACCUM : 0));
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Weight packing (role = forward or data-gradient). Source layouts are the reference's Keras layouts:
// Conv3D (kd,kh,kw,Cin,Cout) -- resnet.py:30-37,80-87; Conv3DTranspose (kd,kh,kw,Cout,Cin) -- upsample.py:28-33.
// The encoder's dense connections feed block j the list [o_{j-1}, o_0..o_{j-1}] (encoder.py:83-87): the
// duplicated slice is folded here (Wp = W[first copy] + W[second copy]) so the kernel reads the level slab
// [o_0..o_{j-1}] once.
// ---------------------------------------------------------------------------------------------
struct PackParams {
  const float* w;
  float* wp;
  int ntaps, K, N, KG, Npad;
  long sT, sK, sN;  // source strides for (tap, k, n)
  int flip;         // tap t reads source tap ntaps-1-t
  int cin_is_k;     // 1: the (possibly folded) input-channel axis is k, 0: it is n, -1: no fold
  int shift, dup_start;
  long wino_off;    // K3S1 images: element index where the Winograd part starts; otherwise beyond the image
  long w3_item0;    // K3S1 images: first work item of the 3-D Winograd part (conv_wino3.hip); its floats start at w3_off
  long w3_off;
  long total;       // floats of the whole image
  long items;       // work items (pack_item): implicit-GEMM floats + Winograd positions (16 floats each), of the parts in `parts` only
  unsigned parts;   // K3S1 images: which of the three parts this pack writes (bit 0 implicit-GEMM, 1 F(2x2,3x3) x direct, 2 F(2x2x2,3x3x3)); 7 = all
};
// index into the items of the enabled parts -> work item of the whole image
__device__ __forceinline__ long pack_map(const PackParams& q, long j) {
  if (q.parts == 7u) return j;
  const long n0 = (q.parts & 1u) ? q.wino_off : 0;
  if (j < n0) return j;
  j -= n0;
  const long n1 = (q.parts & 2u) ? (q.w3_item0 - q.wino_off) : 0;
  if (j < n1) return q.wino_off + j;
  return q.w3_item0 + (j - n1);
}

// source value of packed position (tap t, contraction index k, column n), with the tap flip of the data-gradient role and
// the encoder's duplicated input slice folded in
__device__ __forceinline__ float pack_src(const PackParams& q, int t, int k, int n) {
  if (k >= q.K || n >= q.N) return 0.f;
  const int ts = q.flip ? (q.ntaps - 1 - t) : t;
  int kk = k, nn = n, k2 = -1, n2 = -1;
  if (q.cin_is_k == 1) {
    if (k >= q.dup_start) k2 = k - q.dup_start;
    kk = k + q.shift;
    n2 = n;
  } else if (q.cin_is_k == 0) {
    if (n >= q.dup_start) n2 = n - q.dup_start;
    nn = n + q.shift;
    k2 = k;
  }
  float v = q.w[ts * q.sT + kk * q.sK + nn * q.sN];
  if (q.shift > 0 && k2 >= 0 && n2 >= 0) v += q.w[ts * q.sT + k2 * q.sK + n2 * q.sN];
  return v;
}

// One work item of an image: index i < wino_off writes one float of the implicit-GEMM part; an index above it writes the
// 16 transform points of one (cout block, k-group, x tap, half, cout, cin) position of the Winograd part (conv_wino.hip):
// U = G g G^T over the (z, y) taps, layout [cout block of 32][k-group][x tap][xi_z*4 + xi_y][half][32][4]; the 9 source
// taps are read once.  rows of G: (1 0 0) (.5 .5 .5) (.5 -.5 .5) (0 0 1)
__device__ __forceinline__ float pack_g_(int r, float g0, float g1, float g2) {   // row r of G applied to three taps
  return r == 0 ? g0 : r == 1 ? fmaf(0.5f, g2, fmaf(0.5f, g1, 0.5f * g0)) : r == 2 ? fmaf(0.5f, g2, fmaf(-0.5f, g1, 0.5f * g0)) : g2;
}
__device__ __forceinline__ void pack_item(const PackParams& q, long i) {
  if (i >= q.w3_item0) {
    // third part: U = (G x G x G) g over all 27 taps, 64 transform points xi = (xi_z*4 + xi_y)*4 + xi_x per (cin, cout) pair,
    // layout [cout block of 32][k-group of 8 cin][xi][half][32 couts][4 cin] (conv_wino3.hip)
    long r = i - q.w3_item0;
    const int j = (int)(r & 3);
    const int n32 = (int)((r >> 2) & 31);
    const int hh = (int)((r >> 7) & 1);
    r >>= 8;
    const int kg = (int)(r % q.KG);
    const int cb = (int)(r / q.KG);
    const int k = kg * 8 + hh * 4 + j, n = cb * 32 + n32;
    float t[4][3][3], u[4][4][3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float g0 = pack_src(q, (0 * 3 + ky) * 3 + kx, k, n), g1 = pack_src(q, (1 * 3 + ky) * 3 + kx, k, n),
                    g2 = pack_src(q, (2 * 3 + ky) * 3 + kx, k, n);
#pragma unroll
        for (int a = 0; a < 4; ++a) t[a][ky][kx] = pack_g_(a, g0, g1, g2);
      }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int b = 0; b < 4; ++b) u[a][b][kx] = pack_g_(b, t[a][0][kx], t[a][1][kx], t[a][2][kx]);
    float* o = q.wp + q.w3_off + (((long)cb * q.KG + kg) * 64) * 256 + hh * 128 + n32 * 4 + j;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) o[((a * 4 + b) * 4 + c) * 256] = pack_g_(c, u[a][b][0], u[a][b][1], u[a][b][2]);
    return;
  }
  if (i >= q.wino_off) {
    long r = i - q.wino_off;
    const int j = (int)(r & 3);
    const int n32 = (int)((r >> 2) & 31);
    const int hh = (int)((r >> 7) & 1);
    r >>= 8;
    const int dx = (int)(r % 3); r /= 3;
    const int kg = (int)(r % q.KG);
    const int cb = (int)(r / q.KG);
    const int k = kg * 8 + hh * 4 + j, n = cb * 32 + n32;
    float g[3][3], t[4][3];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) g[kz][ky] = pack_src(q, (kz * 3 + ky) * 3 + dx, k, n);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {  // G along z
      t[0][ky] = g[0][ky];
      t[1][ky] = fmaf(0.5f, g[2][ky], fmaf(0.5f, g[1][ky], 0.5f * g[0][ky]));
      t[2][ky] = fmaf(0.5f, g[2][ky], fmaf(-0.5f, g[1][ky], 0.5f * g[0][ky]));
      t[3][ky] = g[2][ky];
    }
    float* o = q.wp + q.wino_off + ((((long)cb * q.KG + kg) * 3 + dx) * 16) * 256 + hh * 128 + n32 * 4 + j;
#pragma unroll
    for (int xz = 0; xz < 4; ++xz) {  // G along y
      o[(xz * 4 + 0) * 256] = t[xz][0];
      o[(xz * 4 + 1) * 256] = fmaf(0.5f, t[xz][2], fmaf(0.5f, t[xz][1], 0.5f * t[xz][0]));
      o[(xz * 4 + 2) * 256] = fmaf(0.5f, t[xz][2], fmaf(-0.5f, t[xz][1], 0.5f * t[xz][0]));
      o[(xz * 4 + 3) * 256] = t[xz][2];
    }
    return;
  }
  const int j = (int)(i & 3);
  long r = i >> 2;
  const int n = (int)(r % q.Npad); r /= q.Npad;
  const int hh = (int)(r & 1); r >>= 1;
  const int kg = (int)(r % q.KG);
  const int t = (int)(r / q.KG);
  q.wp[i] = pack_src(q, t, kg * 8 + hh * 4 + j, n);
}

__global__ void pack_kernel(const PackParams q) {
  const long total = q.items;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    pack_item(q, pack_map(q, i));
}

// All layers' weight images in one launch (the optimiser step invalidates every image at once; 120 separate 5 us
// launches per training step otherwise).  Descriptor table in device memory, block -> entry by binary search.
#define PACK_BLOCK_ELEMS 2048
struct PackDesc {
  PackParams q;
  long first_block, total;
};
__global__ __launch_bounds__(256) void pack_batch_kernel(const PackDesc* __restrict__ descs, int n) {
  int lo = 0, hi = n - 1;
  const long b = blockIdx.x;
  while (lo < hi) {  // last entry with first_block <= b
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  const PackDesc d = descs[lo];
  const long i0 = (b - d.first_block) * PACK_BLOCK_ELEMS;
#pragma unroll
  for (int u = 0; u < PACK_BLOCK_ELEMS / 256; ++u) {
    const long i = i0 + threadIdx.x + u * 256;
    if (i < d.total) pack_item(d.q, pack_map(d.q, i));
  }
}

static inline int npad32(int n) { return conv_npad32(n); }

extern "C" long bts_conv_packed_floats(int kind, int role, int Cin, int Cout) {
  const int ntaps = (kind == BTS_CONV_K1) ? 1 : 27;
  const int K = (role == BTS_ROLE_FWD) ? Cin : Cout;
  const int N = (role == BTS_ROLE_FWD) ? Cout : Cin;
  // K3S1 images carry two Winograd-domain copies: 16 transform points x 3 x taps (conv_wino.hip), 64 points (conv_wino3.hip)
  return (long)(ntaps + (kind == BTS_CONV_K3S1 ? 48 + 64 : 0)) * ((K + 7) / 8) * 2 * npad32(N) * 4;
}

static int pack_params(PackParams& q, int kind, int role, const float* w, float* wp, int Cin_ref, int Cout, int Cin_slab,
                       int dup_start, int dup_shift, unsigned parts = 7u) {
  if (kind < 0 || kind > 3 || role < 0 || role > 1) return BTS_ERR_UNSUPPORTED;
  if (dup_shift > 0 && (kind == BTS_CONV_K3S2 || kind == BTS_CONV_K3S2T)) return BTS_ERR_UNSUPPORTED;
  if (Cin_slab + dup_shift != Cin_ref) return BTS_ERR_SHAPE;
  q.w = w;
  q.wp = wp;
  q.ntaps = (kind == BTS_CONV_K1) ? 1 : 27;
  q.shift = dup_shift;
  q.dup_start = dup_shift > 0 ? dup_start : (1 << 30);
  long sCin, sCout;
  if (kind == BTS_CONV_K3S2T) { sCout = Cin_ref; sCin = 1; }  // (t, Cout, Cin)
  else { sCin = Cout; sCout = 1; }                            // (t, Cin, Cout)
  q.sT = (long)Cin_ref * Cout;
  if (role == BTS_ROLE_FWD) {
    q.K = Cin_slab; q.N = Cout; q.sK = sCin; q.sN = sCout; q.flip = 0; q.cin_is_k = 1;
  } else {
    q.K = Cout; q.N = Cin_slab; q.sK = sCout; q.sN = sCin; q.cin_is_k = 0;
    q.flip = (kind == BTS_CONV_K3S1) ? 1 : 0;
  }
  q.KG = (q.K + 7) / 8;
  q.Npad = npad32(q.N);
  const long ig = (long)q.ntaps * q.KG * 2 * q.Npad * 4;
  q.wino_off = (kind == BTS_CONV_K3S1) ? ig : (1L << 62);
  const long pairs = (long)q.KG * 2 * q.Npad * 4;   // (contraction index, column) pairs of the padded image
  q.total = ig + ((kind == BTS_CONV_K3S1) ? (48L + 64L) * pairs : 0L);
  q.w3_item0 = (kind == BTS_CONV_K3S1) ? ig + 3L * pairs : (1L << 62);
  q.w3_off = ig + 48L * pairs;
  q.parts = 7u;
  q.items = ig + ((kind == BTS_CONV_K3S1) ? (3L + 1L) * pairs : 0L);
  if (kind == BTS_CONV_K3S1 && (parts & 7u) != 7u && (parts & 7u) != 0u) {
    q.parts = parts & 7u;
    q.items = ((q.parts & 1u) ? ig : 0L) + ((q.parts & 2u) ? 3L * pairs : 0L) + ((q.parts & 4u) ? pairs : 0L);
  }
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Which parts of a K3S1 image are READ.  An image carries three forms of the same weights (139 floats per (cin, cout) pair: 27 + 48 +
// 64) and a layer uses ONE of them at a given geometry -- re-packing all three after every optimiser step wrote ~1.6 GB per fp32
// training step (pack_batch_kernel 0.67-0.77 ms, round-4 review).  The library therefore keeps, per image (keyed by its base address),
// the parts the dispatcher has picked so far (`used`, recorded right before each launch), and descriptor tables are built for those
// parts only (`table_mask`).  A launch that picks a part no table covers packs it on the spot, on its own stream, from the recorded
// source (`fresh_extra` remembers that until the next batch pack, i.e. the next weight change), and bumps the generation counter so that
// the host rebuilds its table (ops.PackTable) at the next re-pack.  bts_conv_pack (single image, all parts) is how images are born.
// ---------------------------------------------------------------------------------------------
#include <mutex>
#include <unordered_map>
struct ImgState {
  int kind, role, Cin_ref, Cout, Cin_slab, dup_start, dup_shift;
  const float* w;
  unsigned used, table_mask, fresh_extra;
};
static std::mutex g_img_mu;
static std::unordered_map<const void*, ImgState> g_img;
static long g_img_gen = 0;
static bool img_masks_enabled() {   // BTS_PACK_USED=0: every pack writes all three parts (A/B; read per call)
  const char* e = getenv("BTS_PACK_USED");
  return !(e && atoi(e) == 0);
}
// (re)register an image; returns the parts a table built now should describe.  table_mask is what the table LAST RUN on the image
// wrote (set by bts_conv_pack_batch from the host copy of that table), never what some table merely describes: with two tables for one
// image, or a cached narrow table behind a bts_conv_pack of the whole image, the parts a batch did NOT write must go stale (round-5
// advisor finding: a re-registration through bts_conv_pack used to mark all three parts as table-covered).
static unsigned img_register(const float* wp, int kind, int role, const float* w, int Cin_ref, int Cout, int Cin_slab, int dup_start,
                             int dup_shift, bool all_parts) {
  std::lock_guard<std::mutex> lk(g_img_mu);
  ImgState& e = g_img[wp];
  const bool same = e.w == w && e.kind == kind && e.role == role && e.Cin_ref == Cin_ref && e.Cout == Cout && e.Cin_slab == Cin_slab &&
                    e.dup_start == dup_start && e.dup_shift == dup_shift;
  if (!same) { e = ImgState{kind, role, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, w, 0u, 0u, 0u}; }      // (another image at this address: nothing is known)
  if (all_parts) {      // bts_conv_pack writes every part: all fresh until the next batch re-pack over this image
    e.fresh_extra = 7u;
    return 7u;
  }
  unsigned m = 7u;
  if (kind == BTS_CONV_K3S1 && e.used != 0u && img_masks_enabled()) m = e.used;
  return m;
}
extern "C" long bts_conv_pack_generation(void) {
  std::lock_guard<std::mutex> lk(g_img_mu);
  return g_img_gen;
}
extern "C" int bts_conv_pack_forget(const float* wp) {      // the image's memory is being released: drop its registry entry
  std::lock_guard<std::mutex> lk(g_img_mu);
  return g_img.erase(wp) ? 1 : 0;
}
__global__ void pack_kernel(const PackParams q);
// Called right before a kernel reads part `bit` of the K3S1 image at `base`: packs the part on `stream` from the recorded source when the
// last re-pack left it out.  The part counts as fresh only after the pack launch was accepted; an error is the caller's to return.
int bts_img_ensure_(const float* base, unsigned bit, hipStream_t stream) {
  PackParams q;
  {
    std::lock_guard<std::mutex> lk(g_img_mu);
    auto it = g_img.find(base);
    if (it == g_img.end() || it->second.kind != BTS_CONV_K3S1) return BTS_OK;      // (an image this registry never saw: packed whole by its owner)
    const ImgState& e = it->second;
    if ((e.table_mask | e.fresh_extra) & bit) return BTS_OK;
    const int r = pack_params(q, e.kind, e.role, e.w, const_cast<float*>(base), e.Cin_ref, e.Cout, e.Cin_slab, e.dup_start, e.dup_shift, bit);
    if (r != BTS_OK) return r;
  }
  long blocks = (q.items + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  (void)hipGetLastError();
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, q);
  BTS_LAUNCH_CHECK();
  std::lock_guard<std::mutex> lk(g_img_mu);
  auto it = g_img.find(base);
  if (it != g_img.end()) it->second.fresh_extra |= bit;
  return BTS_OK;
}
// a launcher has ACCEPTED a launch that reads part `bit`: descriptor tables built from now on describe it (generation moves once per new form)
void bts_img_mark_used_(const float* base, unsigned bit) {
  std::lock_guard<std::mutex> lk(g_img_mu);
  auto it = g_img.find(base);
  if (it == g_img.end() || it->second.kind != BTS_CONV_K3S1) return;
  if (!(it->second.used & bit)) { it->second.used |= bit; ++g_img_gen; }
}

extern "C" int bts_conv_pack(int kind, int role, const float* w, float* wp, int Cin_ref, int Cout, int Cin_slab,
                             int dup_start, int dup_shift, hipStream_t stream) {
  PackParams q;
  const int r = pack_params(q, kind, role, w, wp, Cin_ref, Cout, Cin_slab, dup_start, dup_shift);
  if (r != BTS_OK) return r;
  if (w != nullptr && wp != nullptr) img_register(wp, kind, role, w, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, true);
  const long total = q.items;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  (void)hipGetLastError(); hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(256), 0, stream, q);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" long bts_conv_pack_desc_bytes(void) { return (long)sizeof(PackDesc); }

// Fill descriptor #index of a HOST table (bts_conv_pack_desc_bytes() bytes per entry); first_block = sum of the block
// counts returned for the entries before it.  Returns this entry's block count (> 0) or a negative engine code.
extern "C" long bts_conv_pack_desc(void* host_table, int index, long first_block, int kind, int role, const float* w, float* wp,
                                   int Cin_ref, int Cout, int Cin_slab, int dup_start, int dup_shift) {
  PackDesc d;
  int r = pack_params(d.q, kind, role, w, wp, Cin_ref, Cout, Cin_slab, dup_start, dup_shift);
  if (r != BTS_OK) return r;
  const unsigned parts = img_register(wp, kind, role, w, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, false);   // (the parts read so far; all when none yet)
  if (parts != 7u) r = pack_params(d.q, kind, role, w, wp, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, parts);
  if (r != BTS_OK) return r;
  d.total = d.q.items;
  d.first_block = first_block;
  reinterpret_cast<PackDesc*>(host_table)[index] = d;
  return (d.total + PACK_BLOCK_ELEMS - 1) / PACK_BLOCK_ELEMS;
}

// table_dev: the host table copied to device memory by the caller; table_host: that host table (still readable; may be NULL);
// total_blocks = sum of all block counts.  A batch pack follows a weight change: for every image IN THE TABLE the parts this table
// writes are fresh afterwards and every other part is stale (packed on demand at its next use).  Without the host copy the library cannot
// know which images / parts the table covers: every registered image then counts as stale in every part (correct, but each K3S1 launch
// re-packs its part once per weight change).
extern "C" int bts_conv_pack_batch(const void* table_dev, const void* table_host, int n, long total_blocks, hipStream_t stream) {
  if (n <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffL) return BTS_ERR_SHAPE;
  {
    std::lock_guard<std::mutex> lk(g_img_mu);
    if (table_host != nullptr) {
      const PackDesc* t = reinterpret_cast<const PackDesc*>(table_host);
      for (int i = 0; i < n; ++i) {
        auto it = g_img.find(t[i].q.wp);
        if (it == g_img.end()) continue;
        it->second.table_mask = (it->second.kind == BTS_CONV_K3S1) ? (t[i].q.parts & 7u) : 7u;
        it->second.fresh_extra = 0u;
      }
    } else {
      for (auto& kv : g_img) { kv.second.table_mask = 0u; kv.second.fresh_extra = 0u; }
    }
  }
  (void)hipGetLastError(); hipLaunchKernelGGL(pack_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, stream,
                     reinterpret_cast<const PackDesc*>(table_dev), n);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Transposed-conv gather form with all 8 output-parity classes in ONE workgroup (Conv3DTranspose k3 s2 forward,
// upsample.py:28-33, and the data gradient of the stride-2 conv, downsample.py:28-35).
// out[2c+p] = sum over the taps of parity class p of in[c+d] * W[k]  with per axis  p=0: (k,d) in {(0,0),(2,-1)}, p=1: (1,0).
// The per-class launches of igemm_kernel give the 1-,2- and 4-tap classes 8..32 MFMAs per staged 8-channel slab, far too
// little to cover staging and barriers (51-62 TF).  Here a wave owns 32 coarse voxels and ALL 8 classes: 8 accumulators,
// the 27 taps of a slab need only the 8 input fragments at offsets {-1,0}^3 (8 ds_read_b128 for 108 MFMAs), and the
// tap -> (class, offset) map is compile-time.
// ---------------------------------------------------------------------------------------------
#define UPM_NSLOT 3
static int ilog2(int v);
struct UpmParams {
  const float* x;
  const float* wp;
  const float* bias;
  float* y;
  int N, Di, Hi, Wi, Cin, ldx;  // coarse input grid
  int Cout, ldy, Npad, KG;
  int lgTX, lgTY, TZ, ntx, nty, ntz;
  int IX, IY, IZ;  // halo tile = coarse tile + 1 on the low side of every axis
  int flags;
  float* part;     // split-K partials [ksplit][fine voxel][Npad] (igemm_reduce_kernel finishes them)
  int ksplit, kg_per;
};
__host__ __device__ constexpr int upm_cls(int t) { return ((t / 9 == 1) ? 4 : 0) | (((t / 3) % 3 == 1) ? 2 : 0) | ((t % 3 == 1) ? 1 : 0); }
// halo coordinate of the input voxel per axis: k=2 reads c-1 (index 0), k=0/1 read c (index 1)
__host__ __device__ constexpr int upm_off(int t) { return ((t / 9 == 2) ? 0 : 4) | (((t / 3) % 3 == 2) ? 0 : 2) | ((t % 3 == 2) ? 0 : 1); }

__global__ __launch_bounds__(256, 2) void upm_kernel(const UpmParams p) {
  constexpr int S = 12;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  int b = blockIdx.x;
  const int tx = b % p.ntx; b /= p.ntx;
  const int ty = b % p.nty; b /= p.nty;
  const int tz = b % p.ntz;
  const int n = b / p.ntz;
  const int TX = 1 << p.lgTX, TY = 1 << p.lgTY;
  const int cz0 = tz * p.TZ, cy0 = ty * TY, cx0 = tx * TX;
  const int iz0 = cz0 - 1, iy0 = cy0 - 1, ix0 = cx0 - 1;
  const int tileVox = p.IZ * p.IY * p.IX;
  const int bufDw = tileVox * S;
  const int nslots = tileVox * 2;
  const float* xbase = p.x + ((((long)n * p.Di + iz0) * p.Hi + iy0) * p.Wi + ix0) * (long)p.ldx;
  int goff[UPM_NSLOT];
  const int IYX = p.IY * p.IX;
  const float invIX = 1.0f / (float)p.IX, invIYX = 1.0f / (float)IYX;
#pragma unroll
  for (int i = 0; i < UPM_NSLOT; ++i) {
    const int e = tid + i * 256;
    goff[i] = -1;
    if (e < nslots) {
      const int vox = e >> 1, q = e & 1;
      const int vz = (int)(((float)vox + 0.5f) * invIYX);
      const int r = vox - vz * IYX;
      const int vy = (int)(((float)r + 0.5f) * invIX);
      const int vx = r - vy * p.IX;
      if ((unsigned)(iz0 + vz) < (unsigned)p.Di && (unsigned)(iy0 + vy) < (unsigned)p.Hi && (unsigned)(ix0 + vx) < (unsigned)p.Wi)
        goff[i] = ((vz * p.Hi + vy) * p.Wi + vx) * p.ldx + q * 4;
    }
  }
  const int m = wave * 32 + l32;
  const int mx = m & (TX - 1), my = (m >> p.lgTX) & (TY - 1), mz = m >> (p.lgTX + p.lgTY);
  const int bbase = ((mz * p.IY + my) * p.IX + mx) * S + h * 4;
  int off8[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) off8[o] = ((((o >> 2) & 1) * p.IY + ((o >> 1) & 1)) * p.IX + (o & 1)) * S;
  int ncol = blockIdx.y * 32 + l32;
  if (ncol >= p.Npad) ncol = p.Npad - 1;
  const int lane_woff = (h * p.Npad + ncol) * 4;
  const int wstepKG = 2 * p.Npad * 4, wstepTap = p.KG * wstepKG;

  f32x16 acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  f32x4 pre[UPM_NSLOT];
  auto fetch = [&](int st) {
#pragma unroll
    for (int i = 0; i < UPM_NSLOT; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (goff[i] >= 0) v = *reinterpret_cast<const f32x4*>(xbase + goff[i] + st * 8);
      pre[i] = v;
    }
  };
  auto commit = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < UPM_NSLOT; ++i) {
      const int e = tid + i * 256;
      if (e < nslots) *reinterpret_cast<f32x4*>(buf + (e >> 1) * S + (e & 1) * 4) = pre[i];
    }
  };
  int kgBeg = 0, kgEnd = p.KG;
  if (p.ksplit > 1) {
    kgBeg = blockIdx.z * p.kg_per;
    kgEnd = kgBeg + p.kg_per;
    if (kgEnd > p.KG) kgEnd = p.KG;
  }
  fetch(kgBeg);
  commit(lds);
  __syncthreads();
  for (int st = kgBeg; st < kgEnd; ++st) {
    const float* cur = lds + ((st - kgBeg) & 1) * bufDw;
    const bool more = (st + 1) < kgEnd;
    if (more) fetch(st + 1);
    const float* wk = p.wp + st * wstepKG;  // wave-uniform
    constexpr int AD = 2;
    f32x4 a[AD + 1], bf[8];
#pragma unroll
    for (int q = 0; q < AD; ++q) a[q] = *reinterpret_cast<const f32x4*>((wk + q * wstepTap) + lane_woff);
#pragma unroll
    for (int o = 0; o < 8; ++o) bf[o] = *reinterpret_cast<const f32x4*>(cur + bbase + off8[o]);
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      if (t + AD < 27) a[(t + AD) % (AD + 1)] = *reinterpret_cast<const f32x4*>((wk + (t + AD) * wstepTap) + lane_woff);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[upm_cls(t)] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t % (AD + 1)][j], bf[upm_off(t)][j], acc[upm_cls(t)], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) commit(lds + ((st + 1 - kgBeg) & 1) * bufDw);
    __syncthreads();
  }

  // ---- epilogue: class c = (pz,py,px) writes fine voxel 2*coarse + parity ----
  const int cz = cz0 + mz, cy = cy0 + my, cx = cx0 + mx;
  if (cz >= p.Di || cy >= p.Hi || cx >= p.Wi) return;
  const int nb = blockIdx.y * 32;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int oz = 2 * cz + ((c >> 2) & 1), oy = 2 * cy + ((c >> 1) & 1), ox = 2 * cx + (c & 1);
    const long vfine = (((long)n * (2 * p.Di) + oz) * (2 * p.Hi) + oy) * (2 * p.Wi) + ox;
    if (p.ksplit > 1) {  // raw partial, finished (bias / activation / accumulate) by igemm_reduce_kernel in a fixed order
      float* row = p.part + ((long)blockIdx.z * ((long)p.N * 8 * p.Di * p.Hi * p.Wi) + vfine) * p.Npad;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v4 = {acc[c][4 * g + 0], acc[c][4 * g + 1], acc[c][4 * g + 2], acc[c][4 * g + 3]};
        *reinterpret_cast<f32x4*>(row + nb + 8 * g + 4 * h) = v4;
      }
      continue;
    }
    float* yrow = p.y + vfine * (long)p.ldy;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int co = nb + 8 * g + 4 * h;
      if (co >= p.Cout) continue;
      f32x4 v = {acc[c][4 * g + 0], acc[c][4 * g + 1], acc[c][4 * g + 2], acc[c][4 * g + 3]};
      if (p.flags & IG_FLAG_BIAS) {   // element loads: the bias is a view into the flat parameter buffer, 4-byte aligned only
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += p.bias[co + j];
      }
      if (p.flags & IG_FLAG_SIGMOID) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sigmoidf_(v[j]);
      }
      f32x4* dst = reinterpret_cast<f32x4*>(yrow + co);
      if (p.flags & IG_FLAG_ACCUM) v += *dst;
      *dst = v;
    }
  }
}

// The merged-class kernel takes the all-classes transposed form on 16-byte rows when its halo tile fits the slots and the grid fills the
// chip, or the contraction is long enough to split (deterministic two-stage reduction) and the workspace holds the partials.
static bool upm_accept(const ConvCall& c, ConvChoice& ch) {
  UpmPlan& u = ch.u;
  if ((c.ldx & 3) || (c.ldy & 3) || !c.x16 || !c.y16) return false;
  if ((c.Cin & 7) || (c.Cout & 3) || c.Wi < 8 || c.Hi < 4 || c.Di < 2) return false;
  const int Npad = npad32(c.Cout), KG = c.Cin / 8;
  int TX = 32;
  while (TX > 8 && TX / 2 >= c.Wi) TX /= 2;
  int TY = (TX == 32) ? 2 : 4;
  int TZ = 128 / (TX * TY);
  u.lgTX = ilog2(TX); u.lgTY = ilog2(TY); u.TZ = TZ;
  u.ntx = (c.Wi + TX - 1) / TX; u.nty = (c.Hi + TY - 1) / TY; u.ntz = (c.Di + TZ - 1) / TZ;
  u.IX = TX + 1; u.IY = TY + 1; u.IZ = TZ + 1;
  if (u.IZ * u.IY * u.IX * 2 > 256 * UPM_NSLOT) return false;
  const long wgs = (long)c.N * u.ntz * u.nty * u.ntx * (Npad / 32);
  const long min_wgs = conv_env_long("BTS_IGEMM_UPM_MIN", 256);  // (tests force 1)
  u.ksplit = 1; u.kg_per = KG; u.need = 0;
  if (wgs < min_wgs) {
    // too few workgroups to fill the chip: split the contraction when it is long
    if (KG < 8) return false;
    int ks = (int)((512 + wgs - 1) / wgs);
    if (ks > KG / 4) ks = KG / 4;
    if (ks > 16) ks = 16;
    if (ks < 2) return false;
    u.kg_per = (KG + ks - 1) / ks;
    u.ksplit = (KG + u.kg_per - 1) / u.kg_per;
    if (u.ksplit < 2 || wgs * u.ksplit < min_wgs / 2) return false;
    u.need = (long)u.ksplit * c.N * 8 * c.Di * c.Hi * c.Wi * Npad * 4;
  }
  ch.sym = 20;
  ch.ws = u.need;
  return c.ws_bytes >= u.need;
}

static int launch_upm(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
  const UpmPlan& u = ch.u;
  UpmParams p;
  p.N = c.N; p.Di = c.Di; p.Hi = c.Hi; p.Wi = c.Wi; p.Cin = c.Cin; p.Cout = c.Cout;
  p.Npad = npad32(c.Cout); p.KG = c.Cin / 8;
  p.lgTX = u.lgTX; p.lgTY = u.lgTY; p.TZ = u.TZ; p.ntx = u.ntx; p.nty = u.nty; p.ntz = u.ntz; p.IX = u.IX; p.IY = u.IY; p.IZ = u.IZ;
  p.ksplit = u.ksplit; p.kg_per = u.kg_per;
  p.x = q.x; p.wp = q.wp; p.bias = q.bias; p.y = q.y; p.ldx = c.ldx; p.ldy = c.ldy; p.flags = c.flags;
  p.part = reinterpret_cast<float*>(q.ws);
  const long tiles = (long)c.N * p.ntz * p.nty * p.ntx;
  const int ny = p.Npad / 32;
  const int tileVox = p.IZ * p.IY * p.IX;
  const size_t shmem = (size_t)2 * tileVox * 12 * sizeof(float);
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(20, 2.0 * 27.0 * c.Cin * c.Cout * (double)c.N * c.Di * c.Hi * c.Wi, stream);
  (void)hipGetLastError(); hipLaunchKernelGGL(upm_kernel, dim3((unsigned)tiles, ny, p.ksplit), dim3(256), shmem, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    const long nvox = (long)c.N * 8 * c.Di * c.Hi * c.Wi;
    long blocks = (nvox * c.Cout + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    (void)hipGetLastError(); hipLaunchKernelGGL(igemm_reduce_kernel, dim3((int)blocks), dim3(256), 0, stream, p.part, q.bias, q.y, nvox, c.Cout, p.Npad,
                       c.ldy, p.ksplit, p.flags);
    BTS_LAUNCH_CHECK();
  }
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// 1x1x1 convolution as a streaming GEMM (resnet.py:96-103 shortcut, decoder.py:55-63 output head, vae.py pointwise convs,
// and their data gradients).  These layers are HBM-bound (<= 64 FLOP/B), so nothing is staged: the B fragment of the
// MFMA (voxel l32, channels kg*8 + 4h .. +3) IS a 16-byte global load of that voxel's row, the A fragment the matching
// quad of the packed weights (L1/L2 resident).  A wave owns 64 voxels x 32*NS couts; latency is covered by occupancy
// (~100 VGPRs -> 4 waves per SIMD), not by a software pipeline.
// ---------------------------------------------------------------------------------------------
struct K1sParams {
  const float* x;
  const float* wp;
  const float* bias;
  float* y;
  long nvox;
  int Cin, ldx, Cout, ldy, Npad, KG, flags;
};
template <int NS>
__global__ __launch_bounds__(256, 4) void k1s_kernel(const K1sParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  const long v0 = (long)blockIdx.x * 256 + wave * 64;
  const float* xrow[2];
#pragma unroll
  for (int ms = 0; ms < 2; ++ms) {
    long v = v0 + ms * 32 + l32;
    if (v >= p.nvox) v = p.nvox - 1;  // clamped loads, masked stores
    xrow[ms] = p.x + v * p.ldx + h * 4;
  }
  int woff[NS];
#pragma unroll
  for (int ns = 0; ns < NS; ++ns) {
    int ncol = (blockIdx.y * NS + ns) * 32 + l32;
    if (ncol >= p.Npad) ncol = p.Npad - 1;
    woff[ns] = (h * p.Npad + ncol) * 4;
  }
  const int wstepKG = 2 * p.Npad * 4;
  f32x16 acc[2][NS];
#pragma unroll
  for (int ms = 0; ms < 2; ++ms)
#pragma unroll
    for (int ns = 0; ns < NS; ++ns)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ms][ns][r] = 0.f;
  // U k-groups per step (fewer for the wider tile: 128-VGPR budget), next step's operands requested before this
  // step's MFMAs
  constexpr int U = (NS == 1) ? 2 : 1;
  f32x4 b[2][U][2], a[2][U][NS];
  auto load = [&](int buf, int kg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = (kg + u < p.KG) ? kg + u : p.KG - 1;
#pragma unroll
      for (int ms = 0; ms < 2; ++ms) b[buf][u][ms] = *reinterpret_cast<const f32x4*>(xrow[ms] + k * 8);
#pragma unroll
      for (int ns = 0; ns < NS; ++ns) a[buf][u][ns] = *reinterpret_cast<const f32x4*>((p.wp + k * wstepKG) + woff[ns]);
    }
  };
  auto mma = [&](int buf, int kg) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (kg + u < p.KG) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ms = 0; ms < 2; ++ms)
#pragma unroll
            for (int ns = 0; ns < NS; ++ns)
              acc[ms][ns] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[buf][u][ns][j], b[buf][u][ms][j], acc[ms][ns], 0, 0, 0);
      }
    }
  };
  load(0, 0);
  for (int kg = 0; kg < p.KG; kg += 2 * U) {
    if (kg + U < p.KG) load(1, kg + U);
    mma(0, kg);
    if (kg + U < p.KG) {
      if (kg + 2 * U < p.KG) load(0, kg + 2 * U);
      mma(1, kg + U);
    }
  }
#pragma unroll
  for (int ms = 0; ms < 2; ++ms) {
    const long v = v0 + ms * 32 + l32;
    if (v >= p.nvox) continue;
    float* yrow = p.y + v * p.ldy;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      const int nb = (blockIdx.y * NS + ns) * 32;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co = nb + 8 * g + 4 * h;
        if (co >= p.Cout) continue;
        f32x4 val = {acc[ms][ns][4 * g + 0], acc[ms][ns][4 * g + 1], acc[ms][ns][4 * g + 2], acc[ms][ns][4 * g + 3]};
        if (p.flags & IG_FLAG_BIAS) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co + j < p.Cout) val[j] += p.bias[co + j];
        }
        if (p.flags & IG_FLAG_SIGMOID) {
#pragma unroll
          for (int j = 0; j < 4; ++j) val[j] = sigmoidf_(val[j]);
        }
        if ((p.flags & IG_FLAG_VECOUT) && co + 3 < p.Cout) {
          f32x4* dst = reinterpret_cast<f32x4*>(yrow + co);
          if (p.flags & IG_FLAG_ACCUM) val += *dst;
          *dst = val;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co + j < p.Cout) yrow[co + j] = (p.flags & IG_FLAG_ACCUM) ? yrow[co + j] + val[j] : val[j];
        }
      }
    }
  }
}

// The streaming kernel takes 1x1x1 calls on whole k-groups and 16-byte row quads; small grids (deep levels: too few workgroups) stay
// with the split-K capable staged kernel.
static bool k1s_accept(const ConvCall& c, ConvChoice& ch) {
  if ((c.Cin & 7) || (c.ldx & 3) || !c.x16) return false;
  const long nvox = (long)c.N * c.Di * c.Hi * c.Wi;
  if (nvox < conv_env_long("BTS_IGEMM_K1S_MIN", 256 * 256)) return false;  // (tests force 1)
  ch.sym = 21;
  return (nvox + 255) / 256 <= 0x7fffffffL;
}
static int launch_k1s(const ConvCall& c, const ConvChoice&, const ConvPtrs& q, hipStream_t stream) {
  K1sParams p;
  p.x = q.x; p.wp = q.wp; p.bias = q.bias; p.y = q.y; p.nvox = (long)c.N * c.Di * c.Hi * c.Wi;
  p.Cin = c.Cin; p.ldx = c.ldx; p.Cout = c.Cout; p.ldy = c.ldy; p.Npad = npad32(c.Cout); p.KG = c.Cin / 8;
  p.flags = c.flags;
  if ((c.ldy % 4 == 0) && c.y16) p.flags |= IG_FLAG_VECOUT;
  const long gx = (p.nvox + 255) / 256;
  const bool prof = bts_prof_on();
  const int ns = (p.Npad >= 64) ? 2 : 1;
  if (prof) bts_prof_begin(21, 2.0 * c.Cin * (double)c.Cout * (double)p.nvox, stream);
  (void)hipGetLastError();
  if (ns == 2) hipLaunchKernelGGL(k1s_kernel<2>, dim3((unsigned)gx, (p.Npad + 63) / 64), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(k1s_kernel<1>, dim3((unsigned)gx, 1), dim3(256), 0, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// 3x3x3 stride-1 conv with 1..4 output channels (VAE reconstruction head 32 -> 2, vae.py:92-99 / model.py:72) on the
// vector ALU: padding 2 couts to an MFMA N of 32 wastes 94 % of the matrix pipe (0.99 ms at 128^3).  One output voxel
// per lane; the halo tile is staged 8 channels at a time in the igemm layout (conflict-free ds_read_b128), the
// wave-uniform weights come straight out of the packed image through scalar loads (v_fma with an SGPR operand), so the
// LDS serves only the 2 x 27 activation quads per voxel and slab.  Latency is covered by occupancy (4 workgroups / CU).
// ---------------------------------------------------------------------------------------------
struct DscParams {
  const float* x;
  const float* wp;
  const float* bias;
  float* y;
  int N, D, H, W, Cin, ldx, Cout, ldy, Npad, KG, ntx, nty, ntz, flags;
};
template <int CO>
__global__ __launch_bounds__(256, 4) void dsc_kernel(const DscParams p) {
  constexpr int S = 12, TX = 32, TY = 4, TZ = 2, IX = TX + 2, IY = TY + 2, IZ = TZ + 2;
  constexpr int tileVox = IZ * IY * IX, nslots = tileVox * 2, NSL = (nslots + 255) / 256;
  __shared__ __attribute__((aligned(16))) float lds[tileVox * S];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % p.ntx; b /= p.ntx;
  const int ty = b % p.nty; b /= p.nty;
  const int tz = b % p.ntz;
  const int n = b / p.ntz;
  const int iz0 = tz * TZ - 1, iy0 = ty * TY - 1, ix0 = tx * TX - 1;
  const float* xbase = p.x + ((((long)n * p.D + iz0) * p.H + iy0) * p.W + ix0) * (long)p.ldx;
  int goff[NSL];
#pragma unroll
  for (int i = 0; i < NSL; ++i) {
    const int e = tid + i * 256;
    goff[i] = -1;
    if (e < nslots) {
      const int vox = e >> 1, q = e & 1;
      const int vz = vox / (IY * IX), r = vox - vz * (IY * IX), vy = r / IX, vx = r - vy * IX;
      if ((unsigned)(iz0 + vz) < (unsigned)p.D && (unsigned)(iy0 + vy) < (unsigned)p.H && (unsigned)(ix0 + vx) < (unsigned)p.W)
        goff[i] = ((vz * p.H + vy) * p.W + vx) * p.ldx + q * 4;
    }
  }
  const int mx = tid & (TX - 1), my = (tid >> 5) & (TY - 1), mz = tid >> 7;
  const float* lb = lds + ((mz * IY + my) * IX + mx) * S;
  float acc[CO];
#pragma unroll
  for (int c = 0; c < CO; ++c) acc[c] = 0.f;
  const int wstepKG = 2 * p.Npad * 4, wstepTap = p.KG * wstepKG;
  f32x4 pre[NSL];
  auto fetch = [&](int kg) {
#pragma unroll
    for (int i = 0; i < NSL; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (goff[i] >= 0) v = *reinterpret_cast<const f32x4*>(xbase + goff[i] + kg * 8);
      pre[i] = v;
    }
  };
  fetch(0);
  for (int kg = 0; kg < p.KG; ++kg) {
    __syncthreads();  // previous slab fully consumed
#pragma unroll
    for (int i = 0; i < NSL; ++i) {
      const int e = tid + i * 256;
      if (e < nslots) *reinterpret_cast<f32x4*>(lds + (e >> 1) * S + (e & 1) * 4) = pre[i];
    }
    __syncthreads();
    if (kg + 1 < p.KG) fetch(kg + 1);  // next slab's global loads fly under this slab's arithmetic
    const float* wk = p.wp + kg * wstepKG;  // wave-uniform: scalar loads
    // one x-row of taps (3 taps x 2 halves x CO quads) per scalar-load batch: SMEM returns out of order, so every use
    // of a scalar load drains lgkmcnt to 0 -- batching makes that 9 drains per slab instead of 54
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      float w[3][2][CO * 4];
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int q = 0; q < CO * 4; ++q) w[dx][hh][q] = wk[(r * 3 + dx) * wstepTap + hh * p.Npad * 4 + q];
      f32x4 xv[3][2];
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float* src = lb + (((r / 3) * IY + r % 3) * IX + dx) * S;
        xv[dx][0] = *reinterpret_cast<const f32x4*>(src);
        xv[dx][1] = *reinterpret_cast<const f32x4*>(src + 4);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int c = 0; c < CO; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c] = fmaf(xv[dx][hh][j], w[dx][hh][c * 4 + j], acc[c]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int oz = tz * TZ + mz, oy = ty * TY + my, ox = tx * TX + mx;
  if (oz >= p.D || oy >= p.H || ox >= p.W) return;
  float* yrow = p.y + ((((long)n * p.D + oz) * p.H + oy) * p.W + ox) * (long)p.ldy;
#pragma unroll
  for (int c = 0; c < CO; ++c) {
    if (c < p.Cout) {
      float v = acc[c];
      if (p.flags & IG_FLAG_BIAS) v += p.bias[c];
      if (p.flags & IG_FLAG_SIGMOID) v = sigmoidf_(v);
      if (p.flags & IG_FLAG_ACCUM) v += yrow[c];
      yrow[c] = v;
    }
  }
}

// The direct kernel takes 3x3x3 calls into <= 4 channels on whole k-groups and 16-byte rows when the grid is worth it.
static bool dsc_accept(const ConvCall& c, ConvChoice& ch) {
  if (c.Cout > 4 || (c.Cin & 7) || (c.ldx & 3) || !c.x16) return false;
  const long tiles = (long)c.N * ((c.Di + 1) / 2) * ((c.Hi + 3) / 4) * ((c.Wi + 31) / 32);
  ch.sym = 22;
  return tiles >= conv_env_long("BTS_IGEMM_DSC_MIN", 1024) && tiles <= 0x7fffffffL;  // (tests force 1)
}
static int launch_dsc(const ConvCall& c, const ConvChoice&, const ConvPtrs& q, hipStream_t stream) {
  DscParams p;
  p.x = q.x; p.wp = q.wp; p.bias = q.bias; p.y = q.y;
  p.N = c.N; p.D = c.Di; p.H = c.Hi; p.W = c.Wi; p.Cin = c.Cin; p.ldx = c.ldx; p.Cout = c.Cout; p.ldy = c.ldy;
  p.Npad = npad32(c.Cout); p.KG = c.Cin / 8;
  p.ntx = (c.Wi + 31) / 32; p.nty = (c.Hi + 3) / 4; p.ntz = (c.Di + 1) / 2;
  p.flags = c.flags;
  const long tiles = (long)c.N * p.ntz * p.nty * p.ntx;
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(22, 2.0 * 27.0 * c.Cin * (double)c.Cout * (double)c.N * c.Di * c.Hi * c.Wi, stream);
  (void)hipGetLastError();
  if (c.Cout <= 2) hipLaunchKernelGGL(dsc_kernel<2>, dim3((unsigned)tiles), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(dsc_kernel<4>, dim3((unsigned)tiles), dim3(256), 0, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// 3x3x3 stride-1 conv of a TWO-channel input (the network's first convolutions, model.py / resnet.py:30-37 on the 2ch x 128^3
// volume) into <= 32 output channels.  The tiled kernel pads the 2 channels to a k-group of 8 and runs at a quarter of the
// useful rate; here the contraction index of the MFMA (K = 2) IS the channel pair: one matrix instruction per tap, its B
// operand a single ds_read_b32 of the planar LDS halo tile [channel][z][y][x] (lane = (channel, x)), its A operand the
// tap's 2 x 32 weights held in a register for the whole workgroup.  A wave owns one z plane of the 32 x 4 x 4 tile: the
// 18 input fragments of a kz slab feed the 36 matrix instructions of its four output rows.  Optional second output
// (the 1x1x1 shortcut conv of the same input: one more instruction on the centre fragment), bias, GroupNorm partials.
// ---------------------------------------------------------------------------------------------
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

// The two-channel kernel takes plain 3x3x3 calls (bias at most) into <= 32 channels on 16-byte output rows, with or without the fused
// shortcut output, when the grid is worth it; it writes the GroupNorm partials where the slab groups hold whole 4-plane tiles.
static bool c2_accept(const ConvCall& c, ConvChoice& ch) {
  if (c.Cin != 2 || c.Cout > 32 || c.Cout % 4 != 0 || c.ldy % 4 != 0 || !c.y16) return false;
  if (c.flags & (IG_FLAG_ACCUM | IG_FLAG_SIGMOID)) return false;
  if (c.second == CONV_Y2 && (c.ld2 % 4 != 0 || !c.p2_16)) return false;
  const int nty = (c.Hi + 3) / 4, ntx = (c.Wi + 31) / 32;
  const long tiles = (long)c.N * ((c.Di + 3) / 4) * nty * ntx;
  if (tiles < conv_env_long("BTS_IGEMM_C2_MIN", 512) || tiles > 0x7fffffffL) return false;  // (tests force 1)
  ch.sym = 25;
  ch.gn_B = (long)conv_gn_zt(c, 4) * nty * ntx;
  return true;
}
static int launch_c2(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
  const bool f2 = c.second == CONV_Y2;
  C2Params p;
  p.x = q.x; p.wp = q.wp; p.bias = (c.flags & IG_FLAG_BIAS) ? q.bias : nullptr; p.y = q.y;
  p.wp2 = f2 ? q.wp2 : nullptr; p.bias2 = f2 ? q.bias2 : nullptr; p.y2 = f2 ? q.y2 : nullptr;
  p.N = c.N; p.D = c.Di; p.H = c.Hi; p.W = c.Wi; p.ldx = c.ldx; p.Cout = c.Cout; p.ldy = c.ldy; p.ldy2 = f2 ? c.ld2 : 0; p.Npad = npad32(c.Cout);
  p.ntz = (c.Di + 3) / 4; p.nty = (c.Hi + 3) / 4; p.ntx = (c.Wi + 31) / 32;
  const long tiles = (long)c.N * p.ntz * p.nty * p.ntx;
  p.gnp = ch.gn_B ? q.gnp : nullptr; p.gn_G = ch.gn_B ? c.G : 0; p.gn_zt = ch.gn_B ? (c.Di / c.G) / 4 : 1;
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(25, 2.0 * (27.0 + (f2 ? 1.0 : 0.0)) * c.Cin * (double)c.Cout * (double)c.N * c.Di * c.Hi * c.Wi, stream);
  (void)hipGetLastError();
  if (f2) hipLaunchKernelGGL(c2_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(c2_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Launch logic
// ---------------------------------------------------------------------------------------------
static int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

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
static int igemm_accept(const ConvCall& c, ConvChoice& ch) {
  IgemmPlan& g = ch.g;
  const bool k1 = c.geo == GEO_K1, up = c.geo == GEO_UP, fuse2 = c.second == CONV_Y2;
  const int Do = up ? c.Di : c.Do, Ho = up ? c.Hi : c.Ho, Wo = up ? c.Wi : c.Wo;      // the iteration grid (UP: one parity class)
  const int Npad = npad32(c.Cout), KG = (c.Cin + 7) / 8, KGS = k1 ? 4 : 1;
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
  ch.sym = g.cfg + (k1 ? 8 : 0);
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
  if (p.ksplit > 1) {
    const long nvox = (long)p.N * p.Do * p.Ho * p.Wo;
    long blocks = (nvox * p.Cout + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    (void)hipGetLastError(); hipLaunchKernelGGL(igemm_reduce_kernel, dim3((int)blocks), dim3(256), 0, stream, p.part, p.bias, p.y, nvox, p.Cout,
                       p.Npad, p.ldy, p.ksplit, p.flags);
    BTS_LAUNCH_CHECK();
  }
  return BTS_OK;
}

// The launch igemm_accept planned: the tap tables of the geometry (UP: one per parity class) on the plan's tiles, and the instantiation
// of its config.
static int launch_igemm(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
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
  p.Npad = npad32(c.Cout); p.KG = (c.Cin + 7) / 8;
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

// The kernel of a call, in the order the forms were always offered: 3x3x3 stride 1 -- the direct kernel (no second weight set), the
// two-channel kernel (Cin == 2, no second input), the Winograd forms (never with the sigmoid; the second form then runs as a 1x1x1 launch
// of its own: ch.second -- except the second INPUT of a large unsplit w3 launch, which w3_accept takes into the launch); 1x1x1 -- the streaming kernel; transposed -- the merged-class kernel (both without a second form); then the tiled
// kernel, whose status is that of a call no kernel takes.
static int conv_choose(const ConvCall& c, ConvChoice& ch) {
  ch = ConvChoice{};
  const bool s1 = c.geo == GEO_S1;
  if (s1 && !c.second && dsc_accept(c, ch)) { ch.kernel = CONV_DSC; return BTS_OK; }
  if (s1 && c.Cin == 2 && c.second != CONV_X2 && c2_accept(c, ch)) { ch.kernel = CONV_C2; return BTS_OK; }
  if (s1 && !(c.flags & IG_FLAG_SIGMOID)) {
    ch.second = c.second;
    if (w3_accept(c, ch)) { ch.kernel = CONV_W3; return BTS_OK; }
    if (wino_accept(c, ch)) { ch.kernel = CONV_WINO; return BTS_OK; }
    ch.second = 0;
  }
  if (c.geo == GEO_K1 && !c.second && k1s_accept(c, ch)) { ch.kernel = CONV_K1S; return BTS_OK; }
  if (c.geo == GEO_UP && !c.second && upm_accept(c, ch)) { ch.kernel = CONV_UPM; return BTS_OK; }
  ch.kernel = CONV_IGEMM;
  return igemm_accept(c, ch);
}

// Ensures the image part the chosen kernel reads (3x3x3 stride 1: 1 implicit GEMM and the small-channel kernels | 2 | 4 the Winograd
// forms), launches, and records the part as in use once the launch was accepted.
static int conv_launch(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
  const unsigned bit = c.geo != GEO_S1 ? 0u : ch.kernel == CONV_W3 ? 4u : ch.kernel == CONV_WINO ? 2u : 1u;
  if (bit) { const int e = bts_img_ensure_(q.wp, bit, stream); if (e != BTS_OK) return e; }
  int r;
  switch (ch.kernel) {
    case CONV_DSC: r = launch_dsc(c, ch, q, stream); break;
    case CONV_C2: r = launch_c2(c, ch, q, stream); break;
    case CONV_W3: r = bts_w3_launch_(c, ch, q, stream); break;
    case CONV_WINO: r = bts_wino_launch_(c, ch, q, stream); break;
    case CONV_K1S: r = launch_k1s(c, ch, q, stream); break;
    case CONV_UPM: r = launch_upm(c, ch, q, stream); break;
    default: r = launch_igemm(c, ch, q, stream); break;
  }
  if (r == BTS_OK && bit) bts_img_mark_used_(q.wp, bit);
  return r;
}
// One call of the engine (c's alignment flags come from q; c.ws_bytes = the bytes behind q.ws): chosen -- with the 1x1x1 call a Winograd
// form leaves over -- before anything is packed or launched, then run.  gn_B: the GroupNorm slots written (0: none).
static int conv_run(ConvCall c, const ConvPtrs& q, hipStream_t stream, long* gn_B = nullptr) {
  auto al16 = [](const void* a) { return (((uintptr_t)a) & 15) == 0; };
  c.x16 = al16(q.x); c.y16 = al16(q.y); c.p2_16 = al16(c.second == CONV_Y2 ? (const void*)q.y2 : (const void*)q.x2); c.ws16 = al16(q.ws);
  if (q.ws == nullptr || c.ws_bytes < 0) c.ws_bytes = 0;
  if (gn_B) *gn_B = 0;
  ConvChoice ch, ch2;
  int r = conv_choose(c, ch);
  if (r != BTS_OK) return r;
  ConvCall c2 = c;
  ConvPtrs q2 = {};
  if (ch.second) {
    c2.geo = GEO_K1; c2.second = c2.G = 0; c2.ws_bytes = 0;
    if (ch.second == CONV_Y2) {      // y2 = bias2 + conv1x1x1(x)
      c2.ldy = c.ld2; c2.y16 = c.p2_16; c2.flags = q.bias2 ? IG_FLAG_BIAS : 0;
      q2.x = q.x; q2.wp = q.wp2; q2.bias = q.bias2; q2.y = q.y2;
    } else {                         // y += conv1x1x1(x2)
      c2.ldx = c.ld2; c2.x16 = c.p2_16; c2.flags = IG_FLAG_ACCUM;
      q2.x = q.x2; q2.wp = q.wp2; q2.y = q.y;
    }
    r = conv_choose(c2, ch2);
    if (r != BTS_OK) return r;
  }
  r = conv_launch(c, ch, q, stream);
  if (r == BTS_OK && ch.second) r = conv_launch(c2, ch2, q2, stream);
  if (r == BTS_OK && gn_B) *gn_B = ch.gn_B;
  return r;
}

// The call of a forward (dir 0) or data-gradient (dir 1) entry point; kind, (N, D, H, W, Cin, Cout) and the flags as the ABI names them,
// ldx / ldy: rows of the forward input / output (dir 1: of dx, the tensor written / of dy, the tensor read).  The data gradient of the
// stride-2 conv is the gather form over the fine grid's parity classes, that of the transposed conv the stride-2 'same' conv of dy.
static int conv_call_of(int dir, int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, int flags, ConvCall& c) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || ldx < Cin || ldy < Cout) return BTS_ERR_SHAPE;
  if (kind == BTS_CONV_K3S2 && ((D | H | W) & 1)) return BTS_ERR_SHAPE;  // TF 'same' pads (0,1) only for even sizes
  const bool same = kind == BTS_CONV_K1 || kind == BTS_CONV_K3S1, half = kind == BTS_CONV_K3S2;
  const int Df = same ? D : half ? D / 2 : 2 * D, Hf = same ? H : half ? H / 2 : 2 * H, Wf = same ? W : half ? W / 2 : 2 * W;
  c = ConvCall{};
  c.geo = kind == BTS_CONV_K1 ? GEO_K1 : kind == BTS_CONV_K3S1 ? GEO_S1 : half == (dir == 0) ? GEO_DOWN : GEO_UP;
  c.N = N;
  if (dir == 0) { c.Di = D; c.Hi = H; c.Wi = W; c.Do = Df; c.Ho = Hf; c.Wo = Wf; c.Cin = Cin; c.ldx = ldx; c.Cout = Cout; c.ldy = ldy; }
  else { c.Di = Df; c.Hi = Hf; c.Wi = Wf; c.Do = D; c.Ho = H; c.Wo = W; c.Cin = Cout; c.ldx = ldy; c.Cout = Cin; c.ldy = ldx; }
  if ((flags & BTS_CONV_FLAG_SIGMOID) && dir == 0) c.flags |= IG_FLAG_SIGMOID;
  if (flags & BTS_CONV_FLAG_ACCUM) c.flags |= IG_FLAG_ACCUM;
  return BTS_OK;
}
// the query's view of a call: aligned operands and a workspace as large as needed
static void conv_query_view(ConvCall& c) { c.x16 = c.y16 = c.p2_16 = c.ws16 = 1; c.ws_bytes = LONG_MAX; }
// Workspace for a call on dense operands: the maximum over the kernels that split the contraction and could take the call under some
// switch setting or operand alignment (the Winograd forms may split where the implicit GEMM does not, and vice versa).  For the
// transposed form, whether the merged kernel takes the launch also depends on pointer alignment a query does not have, so its split-K
// requirement is reported as an upper bound (the tiled kernel's parity classes need none).  -1: no kernel takes the call.
static long conv_ws_query(int dir, int kind, int N, int D, int H, int W, int Cin, int Cout) {
  ConvCall c;
  ConvChoice ch;
  if (conv_call_of(dir, kind, N, D, H, W, Cin, Cin, Cout, Cout, 0, c) != BTS_OK) return -1;
  conv_query_view(c);
  if (c.geo == GEO_UP && upm_accept(c, ch) && ch.ws > 0) return ch.ws;
  if (igemm_accept(c, ch) != BTS_OK) return -1;
  long need = ch.ws;
  if (c.geo == GEO_S1) {
    const long wn = wino_ws_need(c), w3 = w3_ws_need(c);
    need = need > wn ? need : wn;
    need = need > w3 ? need : w3;
  }
  return need;
}

// Forward. x:(N,D,H,W,Cin) ld=ldx ; y:(N,Do,Ho,Wo,Cout) ld=ldy with (Do,Ho,Wo) = (D,H,W) | (D/2,..) | (2D,..).
// workspace (may be NULL) enables split-K for grids too small to fill the chip; size from bts_conv3d_fwd_workspace.
extern "C" int bts_conv3d_fwd(int kind, const float* x, const float* wp_fwd, const float* bias, float* y, void* workspace,
                              long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy,
                              int flags, hipStream_t stream) {
  ConvCall c;
  const int r = conv_call_of(0, kind, N, D, H, W, Cin, ldx, Cout, ldy, flags, c);
  if (r != BTS_OK) return r;
  if (bias) c.flags |= IG_FLAG_BIAS;
  c.ws_bytes = workspace_bytes;
  ConvPtrs q = {};
  q.x = x; q.wp = wp_fwd; q.bias = bias; q.y = y; q.ws = workspace;
  return conv_run(c, q, stream);
}
extern "C" long bts_conv3d_fwd_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  return conv_ws_query(0, kind, N, D, H, W, Cin, Cout);
}

// Data gradient. dy has the forward output's shape, dx the forward input's shape (N,D,H,W,Cin).
// wp_bwd is the BTS_ROLE_BWD_DATA packing. flags: BTS_CONV_FLAG_ACCUM adds into dx.
extern "C" int bts_conv3d_bwd_data(int kind, const float* dy, const float* wp_bwd, float* dx, void* workspace,
                                   long workspace_bytes, int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy,
                                   int flags, hipStream_t stream) {
  ConvCall c;
  const int r = conv_call_of(1, kind, N, D, H, W, Cin, lddx, Cout, lddy, flags, c);
  if (r != BTS_OK) return r;
  c.ws_bytes = workspace_bytes;
  ConvPtrs q = {};
  q.x = dy; q.wp = wp_bwd; q.y = dx; q.ws = workspace;
  return conv_run(c, q, stream);
}
extern "C" long bts_conv3d_bwd_data_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  return conv_ws_query(1, kind, N, D, H, W, Cin, Cout);
}

// Fused pair of the ResNet block (resnet.py:118 and :133-134): y = conv3x3x3(x) + bias, y2 = conv1x1x1(x) + bias2 from ONE
// pass over x. wp_fwd: K3S1 forward packing, wp2: K1 forward packing of the shortcut kernel (same Cin/Cout).
// Returns BTS_ERR_UNSUPPORTED when the tiled kernel is the one to take the call and its tiling has no register room for the second
// accumulator set; bts_conv3d_fwd_can_fuse tells beforehand, from the tiled kernel's plan alone (whatever the switches and the
// operands leave to the other kernels): the caller then issues the two convolutions separately.
extern "C" int bts_conv3d_fwd_can_fuse(int N, int D, int H, int W, int Cin, int Cout) {
  ConvCall c;
  ConvChoice ch;
  if (conv_call_of(0, BTS_CONV_K3S1, N, D, H, W, Cin, Cin, Cout, Cout, 0, c) != BTS_OK) return 0;
  conv_query_view(c);
  c.second = CONV_Y2; c.ld2 = Cout;
  return igemm_accept(c, ch) == BTS_OK;
}
extern "C" int bts_conv3d_fwd_fused2(const float* x, const float* wp_fwd, const float* bias, float* y, const float* wp2,
                                     const float* bias2, float* y2, int N, int D, int H, int W, int Cin, int ldx, int Cout,
                                     int ldy, int ldy2, hipStream_t stream) {
  ConvCall c;
  if (conv_call_of(0, BTS_CONV_K3S1, N, D, H, W, Cin, ldx, Cout, ldy, 0, c) != BTS_OK || ldy2 < Cout || !wp2 || !y2) return BTS_ERR_SHAPE;
  if (bias) c.flags |= IG_FLAG_BIAS;
  c.second = CONV_Y2; c.ld2 = ldy2;
  ConvPtrs q = {};
  q.x = x; q.wp = wp_fwd; q.bias = bias; q.y = y; q.wp2 = wp2; q.bias2 = bias2; q.y2 = y2;
  return conv_run(c, q, stream);
}

// ---- convolution + GroupNorm statistics of its output (resnet.py:80-93, downsample.py:41-43: conv -> GroupNormalization) ----
extern "C" long bts_gn_workspace(int N, long V, int C, int G, int mode);
extern "C" int bts_gn_stats(const float* x, float* mean, float* rstd, void* workspace, long workspace_bytes, int N, long V, int C,
                            int G, int mode, float eps, hipStream_t stream);
static long gnfuse_partial_bytes(int N, int Do, int Ho, int Wo, int Cout) {
  // upper bound of N*G*B*2 doubles: one pair per 64-voxel tile and 32-cout tile
  const long tiles = (long)N * ((Do + 0) ) * ((Ho + 3) / 4) * ((Wo + 7) / 8);
  return tiles * ((npad32(Cout) + 31) / 32) * 2 * (long)sizeof(double) + 64;
}
extern "C" long bts_conv3d_fwd_gn_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout, int G) {
  const long cw = bts_conv3d_fwd_workspace(kind, N, D, H, W, Cin, Cout);
  if (cw < 0) return -1;
  int Do = D, Ho = H, Wo = W;
  if (kind == BTS_CONV_K3S2) { Do = D / 2; Ho = H / 2; Wo = W / 2; }
  if (kind == BTS_CONV_K3S2T) { Do = 2 * D; Ho = 2 * H; Wo = 2 * W; }
  const long gw = bts_gn_workspace(N, (long)Do * Ho * Wo, Cout, G, BTS_GN_SLAB);
  if (gw < 0) return -1;
  const long fused = ((cw + 63) & ~63L) + gnfuse_partial_bytes(N, Do, Ho, Wo, Cout);
  return fused > gw ? fused : gw;
}
// y = conv(x) + bias (y dense: ldy == Cout) and (mean, rstd) = slab-mode GroupNorm statistics of y.  The statistics come out
// of the conv epilogue where the chosen kernel writes the partials (ConvChoice::gn_B: no split-K, slab groups of whole tiles);
// otherwise bts_gn_stats runs on y afterwards (same result up to the summation order, both deterministic).
// wp2 != NULL: the fused shortcut pair; the workspace then serves the Winograd forms' split-K on small grids (the fused tiled pair never splits).
static int conv_fwd_gn_impl(int kind, const float* x, const float* wp, const float* bias, float* y, const float* wp2,
                            const float* bias2, float* y2, int ldy2, void* ws, long ws_bytes, int N, int D, int H, int W, int Cin,
                            int ldx, int Cout, int G, float eps, float* mean, float* rstd, hipStream_t stream) {
  if (G <= 0 || Cout % G != 0) return BTS_ERR_SHAPE;
  if (ws == nullptr || ws_bytes < bts_conv3d_fwd_gn_workspace(kind, N, D, H, W, Cin, Cout, G)) return BTS_ERR_WORKSPACE;
  ConvCall c;
  int r = conv_call_of(0, kind, N, D, H, W, Cin, ldx, Cout, Cout, 0, c);
  if (r != BTS_OK) return r;
  if (bias) c.flags |= IG_FLAG_BIAS;
  if (wp2 != nullptr) { c.second = CONV_Y2; c.ld2 = ldy2; }
  const long cw = (bts_conv3d_fwd_workspace(kind, N, D, H, W, Cin, Cout) + 63) & ~63L;
  c.G = G; c.ws_bytes = cw;
  ConvPtrs q = {};
  q.x = x; q.wp = wp; q.bias = bias; q.y = y; q.wp2 = wp2; q.bias2 = bias2; q.y2 = y2; q.ws = ws;
  q.gnp = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + cw);
  long gnB = 0;
  r = conv_run(c, q, stream, &gnB);
  if (r != BTS_OK) return r;
  const long V = (long)c.Do * c.Ho * c.Wo;
  if (gnB > 0) return bts_gn_finalize_partials_(q.gnp, mean, rstd, N * G, gnB, (double)V * Cout / G, eps, stream);
  return bts_gn_stats(y, mean, rstd, ws, ws_bytes, N, V, Cout, G, BTS_GN_SLAB, eps, stream);
}
extern "C" int bts_conv3d_fwd_gn(int kind, const float* x, const float* wp_fwd, const float* bias, float* y, void* workspace,
                                 long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int G, float eps,
                                 float* mean, float* rstd, hipStream_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || ldx < Cin) return BTS_ERR_SHAPE;
  if (((uintptr_t)workspace) & 15) return BTS_ERR_ALIGN;     // (the GroupNorm partials in it are read as double2: refuse before y is written)
  return conv_fwd_gn_impl(kind, x, wp_fwd, bias, y, nullptr, nullptr, nullptr, 0, workspace, workspace_bytes, N, D, H, W, Cin, ldx,
                          Cout, G, eps, mean, rstd, stream);
}
extern "C" int bts_conv3d_fwd_fused2_gn(const float* x, const float* wp_fwd, const float* bias, float* y, const float* wp2,
                                        const float* bias2, float* y2, void* workspace, long workspace_bytes, int N, int D, int H,
                                        int W, int Cin, int ldx, int Cout, int ldy2, int G, float eps, float* mean, float* rstd,
                                        hipStream_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || ldx < Cin || ldy2 < Cout || !wp2 || !y2) return BTS_ERR_SHAPE;
  if (((uintptr_t)workspace) & 15) return BTS_ERR_ALIGN;
  return conv_fwd_gn_impl(BTS_CONV_K3S1, x, wp_fwd, bias, y, wp2, bias2, y2, ldy2, workspace, workspace_bytes, N, D, H, W, Cin, ldx,
                          Cout, G, eps, mean, rstd, stream);
}

// dx (+)= data gradient of a 3x3x3 stride-1 conv (dy, wp_bwd) + data gradient of a 1x1x1 conv of the SAME input (dy2, wp2_bwd):
// the two gradient paths of a ResNet block's input (resnet.py:118,134) in one pass over dx.  Two calls instead where a kernel of the
// 3x3x3 gradient may split the contraction (its workspace answer is not 0) or dy2 cannot be read with 16-byte loads.
extern "C" long bts_conv3d_bwd_data_pair_workspace(int N, int D, int H, int W, int Cin, int Cout) {
  const long a = bts_conv3d_bwd_data_workspace(BTS_CONV_K3S1, N, D, H, W, Cin, Cout);
  const long b = bts_conv3d_bwd_data_workspace(BTS_CONV_K1, N, D, H, W, Cin, Cout);
  if (a < 0 || b < 0) return -1;
  return a > b ? a : b;
}
// The 3x3x3 call of a pair: 1 -- c carries the second input (one engine call), 0 -- c is the plain 3x3x3 call and the 1x1x1 gradient is a
// call of its own, < 0 -- a status.
static int pair_call_of(int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy, int lddy2, int flags, bool dy2_16, ConvCall& c) {
  if (conv_call_of(1, BTS_CONV_K3S1, N, D, H, W, Cin, lddx, Cout, lddy, flags, c) != BTS_OK || lddy2 < Cout) return BTS_ERR_SHAPE;
  const long need = conv_ws_query(1, BTS_CONV_K3S1, N, D, H, W, Cin, Cout);
  if (need < 0) return BTS_ERR_SHAPE;
  const bool fuse = need == 0 && (Cout % 8 == 0) && (lddy2 % 4 == 0) && dy2_16 && Cin > 4 && getenv("BTS_IGEMM_NOPAIR") == nullptr;
  if (fuse) { c.second = CONV_X2; c.ld2 = lddy2; }
  return fuse;
}
// Host only: the convolution launches bts_conv3d_bwd_data_pair makes for the described call (bts_hip.h) -- 1: one kernel forms both
// terms (the tiled kernel, or w3_kernel with the second input in its output side), 2: the 1x1x1 term is a launch of its own.
extern "C" int bts_conv3d_bwd_data_pair_launches(int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy, int lddy2, int flags,
                                                 int aligned, long workspace_bytes) {
  ConvCall c;
  ConvChoice ch;
  const int fuse = pair_call_of(N, D, H, W, Cin, lddx, Cout, lddy, lddy2, flags, (aligned >> 2) & 1, c);
  if (fuse < 0) return fuse;
  if (!fuse) return 2;
  c.x16 = aligned & 1; c.y16 = (aligned >> 1) & 1; c.p2_16 = 1; c.ws16 = (aligned >> 3) & 1;
  c.ws_bytes = workspace_bytes < 0 ? LONG_MAX : workspace_bytes;
  const int r = conv_choose(c, ch);
  return r != BTS_OK ? r : ch.second ? 2 : 1;
}
extern "C" int bts_conv3d_bwd_data_pair(const float* dy, const float* wp_bwd, const float* dy2, const float* wp2_bwd, float* dx,
                                        void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int lddx,
                                        int Cout, int lddy, int lddy2, int flags, hipStream_t stream) {
  ConvCall c;
  const int fuse = pair_call_of(N, D, H, W, Cin, lddx, Cout, lddy, lddy2, flags, (((uintptr_t)dy2) & 15) == 0, c);
  if (fuse < 0) return fuse;
  c.ws_bytes = workspace_bytes;
  ConvPtrs q = {};
  q.x = dy; q.wp = wp_bwd; q.y = dx; q.ws = workspace;
  if (fuse) {
    q.x2 = dy2; q.wp2 = wp2_bwd;
    return conv_run(c, q, stream);
  }
  const int r = conv_run(c, q, stream);
  if (r != BTS_OK) return r;
  return bts_conv3d_bwd_data(BTS_CONV_K1, dy2, wp2_bwd, dx, workspace, workspace_bytes, N, D, H, W, Cin, lddx, Cout, lddy2,
                             flags | BTS_CONV_FLAG_ACCUM, stream);
}

// Which igemm_kernel<...> instantiation the tiled kernel would run a call on: cfg + 8*(KGS==4); cfg ids: IgemmPlan (conv_plan.h).
// Lets the host attribute measured launch times to kernel symbols (bench.py roofline).
static int conv_config_query(int dir, int kind, int N, int D, int H, int W, int Cin, int Cout) {
  ConvCall c;
  ConvChoice ch;
  int r = conv_call_of(dir, kind, N, D, H, W, Cin, Cin, Cout, Cout, 0, c);
  if (r != BTS_OK) return r;
  conv_query_view(c);
  r = igemm_accept(c, ch);
  return r != BTS_OK ? r : ch.sym;
}
extern "C" int bts_conv3d_fwd_config(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  return conv_config_query(0, kind, N, D, H, W, Cin, Cout);
}
extern "C" int bts_conv3d_bwd_data_config(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  return conv_config_query(1, kind, N, D, H, W, Cin, Cout);
}
// The profile symbol of the kernel that takes a call first (host only): 20 upm | 21 k1s | 22 dsc | 25 c2 | 23 wino | 27 w3 | the tiled
// kernel's bts_conv3d_*_config id; a negative value is the status of a call no kernel takes.  Arguments: bts_hip.h.
extern "C" int bts_conv3d_kernel(int dir, int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, int flags, int second,
                                 int ld2, int G, int aligned, long workspace_bytes) {
  ConvCall c;
  ConvChoice ch;
  int r = conv_call_of(dir != 0, kind, N, D, H, W, Cin, ldx, Cout, ldy, flags, c);
  if (r != BTS_OK) return r;
  if (second < 0 || second > CONV_X2 || G < 0) return BTS_ERR_SHAPE;
  if (second && (c.geo != GEO_S1 || ld2 < c.Cout * (second == CONV_Y2) + c.Cin * (second == CONV_X2))) return BTS_ERR_SHAPE;
  c.second = second; c.ld2 = second ? ld2 : 0; c.G = G;
  c.x16 = aligned & 1; c.y16 = (aligned >> 1) & 1; c.p2_16 = (aligned >> 2) & 1; c.ws16 = (aligned >> 3) & 1;
  c.ws_bytes = workspace_bytes < 0 ? LONG_MAX : workspace_bytes;
  r = conv_choose(c, ch);
  return r != BTS_OK ? r : ch.sym;
}
