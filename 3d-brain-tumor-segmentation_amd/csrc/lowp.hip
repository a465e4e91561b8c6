// Reduced-precision STORAGE path of the forward pass (BASELINE configs[4]: full-volume inference in fp16, VAE off; also the
// forward half of configs[2], bf16): activations and packed weights are 16-bit (fp16 or bf16), every sum is fp32 -- conv
// contractions on v_mfma_f32_32x32x16_{f16,bf16}, GroupNorm statistics / SE gates / sigmoid in fp32 from the stored values.
// The fp32 engine (conv_igemm / conv_wino / groupnorm / se) is the parity reference of this path; the reference itself has
// no reduced-precision mode.  Call sites replaced: the same as the fp32 kernels' (layers/resnet.py:116-138,
// group_norm.py:83-124, downsample.py:28-45, upsample.py:28-43, decoder.py:55-63,65-83, encoder.py:69-101, model.py:58-68).
//
// Matrix instruction layout (32x32x16, K = 16 channels): A = weights (row = cout, lane>>5 selects k 0..7 / 8..15: one 16-byte
// load of 8 consecutive input channels), B = activations (column = voxel, same k split: one 16-byte read of 8 consecutive
// channels of the voxel -- NDHWC memory IS the operand layout), D: lane holds voxel lane&31 and couts 8*(r>>2) + 4*(lane>>5)
// + (r&3): four consecutive couts per register quad = one 8-byte store.
//
// This file: the register-staged stride-1 kernel, the split-K finishes, lp_s1_choose (which stride-1 kernel takes a call) and every
// bts_lp_conv3d_* forward and data-gradient entry point.  Weight packing: lowp_pack.hip; casts, samplers and the head: lowp_point.hip;
// GroupNorm: lowp_norm.hip; column sums, the block epilogue and the gate / fused block backward: lowp_block.hip.
//
// The conv kernel of this file:
//   lp_conv_s1_kernel      3x3x3 stride-1 'same' (90 % of the FLOPs): halo tile of 16 channels staged global -> registers ->
//                          LDS (voxel stride 48 bytes: conflict-free 16-byte reads), wave = 32 x-columns x VB rows of one z
//                          plane x CB cout blocks, weights straight from L2 (one fragment feeds VB matrix instructions)
// The 1x1x1, stride-2 and transposed convolutions (and the data gradients on those geometries) live in lowp_gather.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.h"
#include "bts_internal.h"
#include "lowp_common.h"

// =====================================================================================================================
// 3x3x3 stride-1 convolution
// =====================================================================================================================
struct LpS1Params {
  const unsigned short* x;
  const unsigned short* wp;
  const float* bias;
  unsigned short* y;
  int N, D, H, W, ldx, ldy, Cout, KS, NB;   // KS = k-steps of 16 input channels, NB = cout blocks of 32
  int ntx, nty, ntz, ncg;                    // tiles per axis, cout groups of CB blocks
  int ksplit, ks_per;                        // split-K over blockIdx.y (small grids)
  long ntiles;
  int accum;                                 // y += result (gradient accumulation into a slab), else y = result
  float* part;
  double* gnp;                               // fused GroupNorm partial sums of y (slab semantics), [N*G][B][2], B = gn_zt*nty*ntx*ncg; or NULL
  int gn_G, gn_zt;                           // groups; z planes per slab group (D / G)
};
#define LPS 24   // halves per staged voxel: 16 channels + 8 pad (48-byte stride: conflict-free 16-byte reads)

__device__ __forceinline__ u32x2 bload8(__amdgpu_buffer_rsrc_t r, unsigned voff) {
  return __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, 0);
}
__device__ __forceinline__ void bstore8(__amdgpu_buffer_rsrc_t r, unsigned voff, u32x2 v) {
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, 0, 0);
}

template <typename T, int VB, int CB, int TXL>
__global__ __launch_bounds__(256, 2) void lp_conv_s1_kernel(const LpS1Params p) {
  constexpr int TX = 1 << TXL, R = 32 / TX, TY = VB * R, TZ = 4;
  constexpr int SX = TX + 2, SY = TY + 2, SZ = TZ + 2;
  constexpr int NVOX = SX * SY * SZ;
  constexpr int NSLOT = (NVOX * 2 + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  float* const bsh = reinterpret_cast<float*>(lds + NVOX * LPS);     // the tile's 32 * CB bias values (behind the halo tile)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  const int lx = l32 & (TX - 1), ly = l32 >> TXL;
  // Persistent over tiles (blockIdx.x, + gridDim.x, ...), and a tile boundary is a k-step boundary: during a tile's LAST k-step
  // the first halo slab and weight groups of the workgroup's next tile are requested, so the output side below runs with its
  // successor's operands in flight (with 32 input channels a tile has only two k-steps: a fresh global round trip per tile was
  // most of its time).  Everything on the vector-memory queue is issued unconditionally -- masked lanes get an offset outside the
  // buffer descriptor -- so that the compiler's vmcnt waits are exact and the wait for a halo slab never drains the stores issued
  // after it.
  struct Tile { int cg, n, ox0, oy0, oz0; };
  auto coords = [&](long tile) {
    Tile t;
    long b = tile;
    t.cg = (int)(b % p.ncg); b /= p.ncg;
    t.ox0 = (int)(b % p.ntx) * TX; b /= p.ntx;
    t.oy0 = (int)(b % p.nty) * TY; b /= p.nty;
    t.oz0 = (int)(b % p.ntz) * TZ;
    t.n = (int)(b / p.ntz);
    return t;
  };
  __amdgpu_buffer_rsrc_t xr;
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t br = __builtin_amdgcn_make_buffer_rsrc((void*)p.bias, 0, p.bias ? (unsigned)p.Cout * 4u : 0u, 0x00020000);
  unsigned goff[NSLOT];
  // halo origin + per-slot offsets of a tile; slots outside the image get an offset outside the descriptor -> zeros ('same' padding)
  auto setup = [&](const Tile& t) {
    const unsigned short* xorg = p.x + ((((long)t.n * p.D + (t.oz0 - 1)) * p.H + (t.oy0 - 1)) * p.W + (t.ox0 - 1)) * (long)p.ldx;
    xr = __builtin_amdgcn_make_buffer_rsrc((void*)xorg, 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      const int e = tid + i * 256;
      goff[i] = 0x80000000u;
      if (e < NVOX * 2) {
        const int vox = e >> 1, q = e & 1;
        const int vz = vox / (SY * SX);
        const int r = vox - vz * (SY * SX);
        const int vy = r / SX, vx = r - vy * SX;
        if ((unsigned)(t.oz0 - 1 + vz) < (unsigned)p.D && (unsigned)(t.oy0 - 1 + vy) < (unsigned)p.H && (unsigned)(t.ox0 - 1 + vx) < (unsigned)p.W)
          goff[i] = (unsigned)(((vz * p.H + vy) * p.W + vx) * p.ldx + q * 8) * 2u;
      }
    }
  };
  u32x4 pre[NSLOT];
  auto fetch = [&](unsigned soff) {     // soff = k-step * 32 bytes, or 0x80000000: nothing to fetch (zeros, no traffic)
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) pre[i] = bload16(xr, goff[i], soff);
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      const int e = tid + i * 256;
      if (e < NVOX * 2) *reinterpret_cast<u32x4*>(lds + (e >> 1) * LPS + (e & 1) * 8) = pre[i];
    }
  };
  auto bias_of = [&](const Tile& t) {   // thread i < 32*CB holds bias[cout block base + i]; out-of-range -> 0 (one request on every path)
    const int co = t.cg * CB * 32 + tid;
    const unsigned off = (tid < 32 * CB && co < p.Cout) ? (unsigned)co * 4u : 0x80000000u;
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(br, off, 0, 0));
  };
  // this lane's B-operand base inside the tile: voxel (z = wave, y = ly, x = lx), channel half h
  const int bbase = ((wave * SY + ly) * SX + lx) * LPS + h * 8;
  const unsigned wlane = (unsigned)((h * 32 + l32) * 16);
  // k-steps of this workgroup (split-K: blockIdx.y takes k-steps [ks0, ks1))
  int ks0 = 0, ks1 = p.KS;
  if (p.ksplit > 1) {
    ks0 = blockIdx.y * p.ks_per;
    ks1 = ks0 + p.ks_per;
    if (ks1 > p.KS) ks1 = p.KS;
  }
  auto wfrag = [&](int t, int ks, int c, int cg) {
    const int cb = cg * CB + c;
    return bload16(wr, wlane, (unsigned)((((t * p.KS + ks) * p.NB) + (cb < p.NB ? cb : 0)) * 1024));
  };
  constexpr bool ROWS = (R == 1);   // 32-wide tiles: input rows shared by the three dy taps
  // weights: the tap consumed u-th in a k-step (ROWS: (dz, dx) groups of three dy, else plain tap order) lives in a[u % 9] and is
  // requested WT taps ahead (27 % 9 == 0: the slot of a tap is the same in every k-step)
  constexpr int WT = ROWS ? ((CB == 1) ? 6 : 3) : 2;
  u32x4 a[9][CB];
  auto tap_of = [](int u) { return ROWS ? (((u / 9) * 3 + (u % 3)) * 3 + (u / 3) % 3) : u; };   // u -> (dz, dy, dx) tap index
  auto wtap = [&](int u, int ks, int cg) {
#pragma unroll
    for (int c = 0; c < CB; ++c) a[u % 9][c] = wfrag(tap_of(u), ks, c, cg);
  };

  f32x16 acc[VB][CB];
  long tile = blockIdx.x;
  if (tile >= p.ntiles) return;
  Tile cur = coords(tile);
  setup(cur);
  float bias_v = bias_of(cur);
  fetch((unsigned)ks0 * 32u);
#pragma unroll
  for (int u = 0; u < WT; ++u) wtap(u, ks0, cur.cg);
  for (; tile < p.ntiles; tile += gridDim.x) {
    const bool have_next = tile + gridDim.x < p.ntiles;
    const Tile nxt = have_next ? coords(tile + gridDim.x) : cur;
#pragma unroll
    for (int v = 0; v < VB; ++v)
#pragma unroll
      for (int c = 0; c < CB; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[v][c][r] = 0.f;
    for (int ks = ks0; ks < ks1; ++ks) {
      __syncthreads();        // every wave is done reading the previous k-step's tile (and the previous tile's bias)
      commit();
      if (ks == ks0 && tid < 32 * CB) bsh[tid] = bias_v;
      __syncthreads();
      const bool last = ks + 1 == ks1;
      if (last && have_next) {   // from here on the input-side state is the next tile's
        setup(nxt);
        bias_v = bias_of(nxt);
      } else {
        bias_v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(br, 0x80000000u, 0, 0));   // (same request count)
      }
      fetch(last ? (have_next ? (unsigned)ks0 * 32u : 0x80000000u) : (unsigned)(ks + 1) * 32u);
      const int ksn = last ? ks0 : ks + 1;
      const int cgn = last ? nxt.cg : cur.cg;
      if constexpr (ROWS) {
        // the input rows of group g+1 are read while group g computes -- where the registers allow it (4 x 2 tiles: 128 accumulators
        // + weight ring + halo prefetch leave room for one row set only)
        constexpr int NB_ = (VB * CB >= 8) ? 1 : 2;
        u32x4 bj[NB_][VB + 2];
        auto rows = [&](u32x4 (&dst)[VB + 2], int g) {
          const int dz = g / 3, dx = g % 3;
#pragma unroll
          for (int j = 0; j < VB + 2; ++j) dst[j] = *reinterpret_cast<const u32x4*>(lds + bbase + ((dz * SY + j) * SX + dx) * LPS);
        };
        if (NB_ == 2) rows(bj[0], 0);
#pragma unroll
        for (int u = 0; u < 27; ++u) {
          const int g = u / 3, dy = u % 3;
          if (u + WT < 27) wtap(u + WT, ks, cur.cg); else wtap(u + WT - 27, ksn, cgn);
          if (dy == 0) { if (NB_ == 2) { if (g + 1 < 9) rows(bj[(g + 1) % NB_], g + 1); } else rows(bj[0], g); }
#pragma unroll
          for (int v = 0; v < VB; ++v)
#pragma unroll
            for (int c = 0; c < CB; ++c) acc[v][c] = T::mfma(a[u % 9][c], bj[g % NB_][v + dy], acc[v][c]);
        }
      } else {
#pragma unroll
        for (int t = 0; t < 27; ++t) {
          const int dz = t / 9, dy = (t / 3) % 3, dx = t % 3;
          if (t + WT < 27) wtap(t + WT, ks, cur.cg); else wtap(t + WT - 27, ksn, cgn);
#pragma unroll
          for (int v = 0; v < VB; ++v) {
            const u32x4 bv = *reinterpret_cast<const u32x4*>(lds + bbase + ((dz * SY + (v * R + dy)) * SX + dx) * LPS);
#pragma unroll
            for (int c = 0; c < CB; ++c) acc[v][c] = T::mfma(a[t % 9][c], bv, acc[v][c]);
          }
        }
      }
    }
    // ---- output side of `cur` ----
    const int oz = cur.oz0 + wave, ox = cur.ox0 + lx;
    const bool gn_on = p.gnp != nullptr;
    float gn_s = 0.f, gn_q = 0.f;
    if (p.ksplit > 1) {   // raw fp32 partial sums [split][voxel][NB*32]; bias / rounding happen in the reduce kernel
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const int cb = cur.cg * CB + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int v = 0; v < VB; ++v) {
            const int oy = cur.oy0 + v * R + ly;
            if (cb < p.NB && oz < p.D && oy < p.H && ox < p.W) {
              float* dst = p.part + ((((long)blockIdx.y * p.N + cur.n) * p.D + oz) * p.H + oy) * (long)p.W * (p.NB * 32) +
                           (long)ox * (p.NB * 32) + cb * 32 + 8 * q + 4 * h;
              *reinterpret_cast<f32x4*>(dst) = f32x4{acc[v][c][4 * q], acc[v][c][4 * q + 1], acc[v][c][4 * q + 2], acc[v][c][4 * q + 3]};
            }
          }
        }
      }
    } else if (p.Cout % 4 == 0) {
      // bias from LDS, convert, one 8-byte buffer store per register quad (masked positions out of range)
      const __amdgpu_buffer_rsrc_t yr =
          __builtin_amdgcn_make_buffer_rsrc((void*)(p.y + (long)cur.n * p.D * p.H * p.W * (long)p.ldy), 0, 0x7fffffff, 0x00020000);
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const int cb = cur.cg * CB + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int co = cb * 32 + 8 * q + 4 * h;
          const f32x4 bq = *reinterpret_cast<const f32x4*>(bsh + c * 32 + 8 * q + 4 * h);
#pragma unroll
          for (int v = 0; v < VB; ++v) {
            const int oy = cur.oy0 + v * R + ly;
            const bool ok = cb < p.NB && co < p.Cout && oz < p.D && oy < p.H && ox < p.W;
            const unsigned off = ok ? (unsigned)((((oz * p.H + oy) * p.W + ox) * p.ldy + co) * 2) : 0x80000000u;
            float o0 = acc[v][c][4 * q] + bq[0], o1 = acc[v][c][4 * q + 1] + bq[1], o2 = acc[v][c][4 * q + 2] + bq[2],
                  o3 = acc[v][c][4 * q + 3] + bq[3];
            if (p.accum) {
              const u32x2 old = bload8(yr, off);
              o0 += T::ld((unsigned short)(old[0] & 0xffffu)); o1 += T::ld((unsigned short)(old[0] >> 16));
              o2 += T::ld((unsigned short)(old[1] & 0xffffu)); o3 += T::ld((unsigned short)(old[1] >> 16));
            }
            bstore8(yr, off, u32x2{pack2<T>(o0, o1), pack2<T>(o2, o3)});
            if (gn_on && ok) {   // (gn_on is launch-uniform) the unrounded outputs: what the stored values estimate
              gn_s += (o0 + o1) + (o2 + o3);
              gn_q = fmaf(o0, o0, fmaf(o1, o1, fmaf(o2, o2, fmaf(o3, o3, gn_q))));
            }
          }
        }
      }
      if (gn_on) {   // one fp64 (sum, sumsq) pair per (z plane = wave, tile column, cout group): lanes by shuffle tree, fixed order
        const double ds = wave_sum_f64((double)gn_s), dq = wave_sum_f64((double)gn_q);
        if (lane == 0 && oz < p.D) {
          const int ty = cur.oy0 / TY, tx = cur.ox0 / TX;
          const int gg = oz / p.gn_zt;      // gn_zt = planes per z-slab group
          const long B = (long)p.gn_zt * p.nty * p.ntx * p.ncg;
          const long slot = (((long)(oz - gg * p.gn_zt) * p.nty + ty) * p.ntx + tx) * p.ncg + cur.cg;
          double* dst = p.gnp + (((long)cur.n * p.gn_G + gg) * B + slot) * 2;
          dst[0] = ds;
          dst[1] = dq;
        }
      }
    } else {
      // heads with fewer than four output channels per quad: element-wise stores
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const int cb = cur.cg * CB + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int co = cb * 32 + 8 * q + 4 * h;
          const f32x4 bq = *reinterpret_cast<const f32x4*>(bsh + c * 32 + 8 * q + 4 * h);
#pragma unroll
          for (int v = 0; v < VB; ++v) {
            const int oy = cur.oy0 + v * R + ly;
            if (cb < p.NB && oz < p.D && oy < p.H && ox < p.W && co < p.Cout) {
              unsigned short* dst = p.y + ((((long)cur.n * p.D + oz) * p.H + oy) * p.W + ox) * (long)p.ldy + co;
              lp_store_quad<T>(dst, acc[v][c][4 * q] + bq[0], acc[v][c][4 * q + 1] + bq[1], acc[v][c][4 * q + 2] + bq[2],
                               acc[v][c][4 * q + 3] + bq[3], p.Cout - co, p.accum);
            }
          }
        }
      }
    }
    cur = nxt;
  }
}

// finish of a split-K launch: y = round(bias + sum_z part[z]) in fixed order
template <typename T>
__global__ __launch_bounds__(256) void lp_splitk_reduce_kernel(const float* part, const float* bias, unsigned short* y, long nvox, int Cout,
                                                               int Npad, int ldy, int ksplit, int accum) {
  const int q4 = Npad / 4;
  const long total = nvox * q4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long v = i / q4;
    const int c = (int)(i - v * q4) * 4;
    if (c >= Cout) continue;
    f32x4 s = *reinterpret_cast<const f32x4*>(part + v * Npad + c);
    for (int z = 1; z < ksplit; ++z) s += *reinterpret_cast<const f32x4*>(part + ((long)z * nvox + v) * Npad + c);
    if (bias) {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (c + j < Cout) s[j] += bias[c + j];
    }
    lp_store_quad<T>(y + v * ldy + c, s[0], s[1], s[2], s[3], Cout - c, accum);
  }
}

// The same finish for a conv whose output goes into a slab-mode GroupNorm (dense y, Cout % 32 == 0): the workgroups walk the (sample, slab)
// units the way lp_gn_stats_kernel does and leave (sum, sumsq) partials of the ROUNDED values, like that kernel -- the statistics pass over
// the stored tensor and its launch go away (the deepest level of the inference volume runs eight such layers).
template <typename T>
__global__ __launch_bounds__(256) void lp_splitk_reduce_gn_kernel(const float* part, const float* bias, unsigned short* y, double* gn_partial,
                                                                  long nvox, long E, long L, int C, int G, int ksplit, int B) {
  __shared__ double sh[8];
  const int unit = blockIdx.y, n = unit / G, g = unit % G;
  const long lo = (long)n * E + (long)g * L;
  const long per = ((L / 8 + B - 1) / B) * 8;
  const long a = lo + (long)blockIdx.x * per, bnd = (a + per < lo + L) ? a + per : lo + L;
  const long tot = nvox * C;
  double s = 0.0, q = 0.0;
  float fs = 0.f, fq = 0.f;
  long cnt = 0;
  for (long i = a + threadIdx.x * 8L; i < bnd; i += 256 * 8) {
    const int c = (int)(i % C);
    f32x4 u0 = *reinterpret_cast<const f32x4*>(part + i), u1 = *reinterpret_cast<const f32x4*>(part + i + 4);
    for (int z = 1; z < ksplit; ++z) {
      u0 += *reinterpret_cast<const f32x4*>(part + (long)z * tot + i);
      u1 += *reinterpret_cast<const f32x4*>(part + (long)z * tot + i + 4);
    }
    float o[8], v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = u0[e]; o[4 + e] = u1[e]; }
    if (bias) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += bias[c + e];
    }
    const u32x4 r = pack8<T>(o);
    *reinterpret_cast<u32x4*>(y + i) = r;
    unpack8<T>(r, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) { fs += v[e]; fq = fmaf(v[e], v[e], fq); }
    if (++cnt == 64) { s += fs; q += fq; fs = fq = 0.f; cnt = 0; }
  }
  s += fs; q += fq;
  s = block_sum_f64(s, sh);
  q = block_sum_f64(q, sh + 4);
  if (threadIdx.x == 0) {
    double* o = gn_partial + ((long)unit * B + blockIdx.x) * 2;
    o[0] = s; o[1] = q;
  }
}
// partial slots per (n, group) the kernel above leaves (0 = it does not take the shape)
long bts_lp_splitk_gn_B_(int N, long V, int Cout, int G) {
  if (G <= 0 || Cout % 32 != 0 || Cout % G != 0 || (V * Cout) % G != 0 || ((V * Cout) / G) % 8 != 0) return 0;
  // (many short workgroups -- one or two 2048-element steps each: the tensor is small and the pass is latency-bound; < 512 partials per
  // unit keeps the finalize on its one-wave-per-unit form)
  long b = (V * Cout / G + 2047) / 2048;
  if (b > 448) b = 448;
  return b;
}
int bts_lp_splitk_reduce_gn_(int dtype, const float* part, const float* bias, void* y, double* gn_partial, int N, long V, int Cout, int G,
                             int ksplit, hipStream_t stream) {
  const long B = bts_lp_splitk_gn_B_(N, V, Cout, G);
  if (B <= 0 || (((uintptr_t)y) & 15)) return BTS_ERR_UNSUPPORTED;
  const long E = V * Cout, L = E / G;
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(lp_splitk_reduce_gn_kernel<T>, dim3((unsigned)B, (unsigned)(N * G)), dim3(256), 0, stream, part, bias, (unsigned short*)y,
                       gn_partial, (long)N * V, E, L, Cout, G, ksplit, (int)B);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

int bts_lp_splitk_reduce_(int dtype, const float* part, const float* bias, void* y, long nvox, int Cout, int Npad, int ldy, int ksplit,
                          int accum, hipStream_t stream) {
  long blocks = (nvox * (Npad / 4) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(lp_splitk_reduce_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, part, bias, (unsigned short*)y, nvox, Cout, Npad, ldy,
                       ksplit, accum);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// split-K plan of the stride-1 kernel: grids that cannot give every CU a workgroup split the input channels
static int lp_s1_ksplit(long wgs, int KS) {
  if (wgs >= 192 || KS < 8) return 1;
  int ks = (int)((384 + wgs - 1) / wgs);
  if (ks > KS / 4) ks = KS / 4;    // at least 4 k-steps per workgroup
  if (ks > 16) ks = 16;
  return ks < 1 ? 1 : ks;
}

template <typename T, int VB, int CB, int TXL>
static int lp_s1_launch(const LpS1Params& p, hipStream_t stream) {
  constexpr int TX = 1 << TXL, R = 32 / TX, TY = VB * R, TZ = 4;
  const long nvox = (long)p.N * p.D * p.H * p.W;
  const size_t shmem = (size_t)(TX + 2) * (TY + 2) * (TZ + 2) * LPS * 2 + 32 * CB * 4;   // halo tile + the tile's bias values
  auto kern = lp_conv_s1_kernel<T, VB, CB, TXL>;
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  (void)hipGetLastError();
  const long grid = p.ntiles < 1024 ? p.ntiles : 1024;   // <= 4 workgroups per CU in flight or queued
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(30, 2.0 * 27.0 * 16.0 * p.KS * p.Cout * (double)nvox, stream);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid, p.ksplit), dim3(256), shmem, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    long blocks = (nvox * (p.NB * 8) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(lp_splitk_reduce_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, p.part, p.bias, p.y, nvox, p.Cout, p.NB * 32,
                       p.ldy, p.ksplit, p.accum);
    BTS_LAUNCH_CHECK();
  }
  return BTS_OK;
}

// (VB, CB, TXL) of a stride-1 call
static void lp_s1_shape(int N, int D, int H, int W, int NB, int& vb, int& cb, int& txl) {
  // x extent of a wave's 32 columns: the widest power of two that wastes no more columns than a narrower one would
  txl = (W >= 24) ? 5 : (W >= 12 ? 4 : 3);
  // rows per wave (VB) and cout blocks per wave (CB): 4 x 1 for 32-cout layers (one weight fragment feeds 4 matrix
  // instructions), 4 x 2 from 64 couts on.  Small grids keep the 4 rows (weight reuse) and split the input channels instead
  cb = NB >= 2 ? 2 : 1;
  const long vox = (long)N * D * H * W;
  vb = vox >= 4096 ? 4 : (vox >= 1024 ? 2 : 1);
  if (vb == 4 && txl == 5) cb = 1;   // 4 x 2 tiles (128 accumulators + weight ring + halo prefetch) spill at two waves per SIMD
}
bool lp_s1_accept(const LpS1Call& c, LpS1Choice& ch) {
  LpS1Shape& s = ch.s;
  const int NB = (c.Cout + 31) / 32, KS = c.Cin / 16;
  lp_s1_shape(c.N, c.D, c.H, c.W, NB, s.vb, s.cb, s.txl);
  const int TX = 1 << s.txl, TY = s.vb * (32 / TX);
  s.ntx = (c.W + TX - 1) / TX; s.nty = (c.H + TY - 1) / TY; s.ntz = (c.D + 3) / 4; s.ncg = (NB + s.cb - 1) / s.cb;
  s.wgs = (long)c.N * s.ntz * s.nty * s.ntx * s.ncg;
  if (s.wgs > 0x7fffffffL) return false;
  if ((long)c.D * c.H * c.W * (long)c.ldy * 2 >= 0x7fffff00L) return false;   // 31-bit output offsets inside one sample
  const int ks = lp_s1_ksplit(s.wgs, KS);
  s.ks_per = (KS + ks - 1) / ks;
  s.ksplit = (KS + s.ks_per - 1) / s.ks_per;
  ch.ws = ks > 1 ? (long)ks * c.N * c.D * c.H * c.W * NB * 32 * 4 : 0;      // (sized for the split before rounding, as it always was)
  // GroupNorm partials from the epilogue: no split-K, whole planes per group, four-cout stores
  ch.B = (c.G > 0 && !c.gnb_G && s.ksplit == 1 && c.D % c.G == 0 && c.Cout % 4 == 0) ? (long)(c.D / c.G) * s.nty * s.ntx * s.ncg : 0;
  return true;
}

template <typename T>
static int lp_s1_dispatch(const LpS1Call& c, const LpS1Choice& ch, const LpS1Ptrs& q, hipStream_t stream) {
  const LpS1Shape& s = ch.s;
  LpS1Params p;
  p.x = (const unsigned short*)q.x; p.wp = (const unsigned short*)q.wp; p.bias = q.bias; p.y = (unsigned short*)q.y;
  p.N = c.N; p.D = c.D; p.H = c.H; p.W = c.W; p.ldx = c.ldx; p.ldy = c.ldy; p.Cout = c.Cout; p.KS = c.Cin / 16; p.NB = (c.Cout + 31) / 32;
  p.accum = c.accum;
  p.gnp = q.gnp; p.gn_G = q.gnp != nullptr ? c.G : 0; p.gn_zt = p.gn_G > 0 ? c.D / p.gn_G : 1;
  p.ntx = s.ntx; p.nty = s.nty; p.ntz = s.ntz; p.ncg = s.ncg; p.ntiles = s.wgs;
  p.ksplit = s.ksplit; p.ks_per = s.ks_per;
  p.part = reinterpret_cast<float*>(q.ws);
  const long nvox = (long)c.N * c.D * c.H * c.W;
  if (p.ksplit > 1 && (q.ws == nullptr || q.ws_bytes < (long)p.ksplit * nvox * p.NB * 32 * 4 || (((uintptr_t)q.ws) & 15))) { p.ksplit = 1; p.ks_per = p.KS; }
#define LP_S1_CASE(VB_, CB_, TXL_) if (s.vb == VB_ && s.cb == CB_ && s.txl == TXL_) return lp_s1_launch<T, VB_, CB_, TXL_>(p, stream);
  LP_S1_CASE(4, 1, 5) LP_S1_CASE(4, 2, 5) LP_S1_CASE(2, 1, 5) LP_S1_CASE(2, 2, 5) LP_S1_CASE(1, 1, 5) LP_S1_CASE(1, 2, 5)
  LP_S1_CASE(4, 1, 4) LP_S1_CASE(4, 2, 4) LP_S1_CASE(2, 1, 4) LP_S1_CASE(2, 2, 4) LP_S1_CASE(1, 1, 4) LP_S1_CASE(1, 2, 4)
  LP_S1_CASE(4, 1, 3) LP_S1_CASE(4, 2, 3) LP_S1_CASE(2, 1, 3) LP_S1_CASE(2, 2, 3) LP_S1_CASE(1, 1, 3) LP_S1_CASE(1, 2, 3)
#undef LP_S1_CASE
  return BTS_ERR_UNSUPPORTED;
}

// The stride-1 kernel of a call: the z-marching kernel (lowp_s1z.hip) for few channels on a big volume, then the LDS-DMA tiled one
// (lowp_s1d.hip), then the register-staged one.  Forms: GroupNorm-backward class sums (gnb), GroupNorm applied to the input (gna),
// FS and a second input tensor (ldxb) only on the first, a split output only on the second, SC on the first two.  G and gnb are
// epilogues: the kernel that takes the plain call writes them, or nobody does (B = 0).
int lp_s1_choose(const LpS1Call& c, LpS1Choice& ch) {
  ch = LpS1Choice{};
  if (c.N <= 0 || c.D <= 0 || c.H <= 0 || c.W <= 0 || c.Cin <= 0 || c.Cout <= 0) return BTS_ERR_SHAPE;
  if (c.Cin % 16 != 0 || c.ldx % 8 != 0 || c.ldx < (c.ldxb ? 32 : c.Cin) || c.ldy < (c.ysplit ? 32 : c.Cout) || (c.Cout >= 4 && c.ldy % 4 != 0))
    return BTS_ERR_ALIGN;
  if (((long)(c.D + 2) * c.H * c.W + 64) * (long)c.ldx * 2 >= 0x7fffffffL) return BTS_ERR_SHAPE;   // 31-bit offsets inside one volume
  // BTS_LP_SC=0 / BTS_LP_FS=0: never the SC / FS form (A/B; read once)
  static const bool sc_off = [] { const char* e = getenv("BTS_LP_SC"); return e && atoi(e) == 0; }();
  static const bool fs_off = [] { const char* e = getenv("BTS_LP_FS"); return e && atoi(e) == 0; }();
  const bool z_only = c.gna_G || c.Cout2 || c.ldxb;
  if (!(c.ldx2 && sc_off) && !(c.Cout2 && fs_off)) {
    if (!c.ysplit && lp_s1z_accept(c, ch)) { ch.kernel = LP_S1Z; return BTS_OK; }
    if (!z_only && lp_s1d_accept(c, ch)) { ch.kernel = LP_S1D; return BTS_OK; }
    if (!z_only && !c.ysplit && !c.ldx2 && lp_s1_accept(c, ch)) { ch.kernel = LP_S1; return BTS_OK; }
  }
  if (!(z_only || c.ysplit || c.ldx2)) return BTS_ERR_SHAPE;
  LpS1Call plain = c;
  plain.gna_G = plain.ldx2 = plain.Cout2 = plain.ldy2 = plain.ldxb = 0;
  plain.ysplit = 0;
  const int r = lp_s1_choose(plain, ch);
  return r == BTS_OK ? 1 : r;
}
int lp_s1_run(int dtype, const LpS1Call& c, const LpS1Choice& ch, LpS1Ptrs q, hipStream_t stream) {
  if (ch.kernel == LP_S1) return lp_typed(dtype, [&](auto t) { return lp_s1_dispatch<decltype(t)>(c, ch, q, stream); });
  q.wp = reinterpret_cast<const char*>(q.wp) + lp_s1d_part_offset(c.Cin, c.Cout);      // (the DMA part of the image)
  return ch.kernel == LP_S1Z ? bts_lp_s1z_launch_(dtype, c, ch, q, stream) : bts_lp_s1d_launch_(dtype, c, ch, q, stream);
}

// geometry-driven core of both entry points below.  geo: 0 = 1x1x1, 1 = 3x3x3 stride 1, 2 = stride-2 gather (out = ceil(in/2),
// in = 2o + k - pad), 3 = 8 output-parity classes of the transposed form (out = 2 in; even outputs take (i, k=0) and (i-1, k=2),
// odd ones (i, k=1)).  (D,H,W) are the dims of `x`, the tensor the taps read; Cin its channels (the contraction).  Every geometry but 1: lowp_gather.hip.
static int lp_conv_run(int geo, int dtype, const void* x, const void* wp, const float* bias, void* y, void* workspace, long workspace_bytes,
                       int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, int accum, hipStream_t stream) {
  const LpGPtrs gq{x, wp, bias, y};
  LpGChoice gch;
  if (geo != 1) return bts_lp_g_conv_(dtype, LpGCall{geo, N, D, H, W, Cin, ldx, Cout, ldy, accum}, &gq, 0, gch, stream);
  const int chk = lp_conv_check(dtype, x, wp, y, N, D, H, W, Cin, ldx, Cout, ldy);
  if (chk != BTS_OK) return chk;
  LpS1Call c = lp_s1_call(N, D, H, W, Cin, Cout);
  c.ldx = ldx; c.ldy = ldy; c.accum = accum; c.aligned = lp_al16(x) && lp_al16(y) && lp_al16(wp);
  LpS1Choice ch;
  const int r = lp_s1_choose(c, ch);
  if (r != BTS_OK) return r;
  return lp_s1_run(dtype, c, ch, LpS1Ptrs{x, wp, bias, y, workspace, workspace_bytes}, stream);
}

static long lp_s1_workspace(int N, int D, int H, int W, int Cin, int Cout) {
  LpS1Choice ch;
  return lp_s1_choose(lp_s1_call(N, D, H, W, Cin, Cout), ch) == BTS_OK ? ch.ws : 0;
}
extern "C" long bts_lp_conv3d_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  return kind == BTS_CONV_K3S1 ? lp_s1_workspace(N, D, H, W, Cin, Cout) : 0;
}
// y = conv(x) + bias in the storage type.  x (N,D,H,W,Cin) stride ldx (elements); y (N,D',H',W',Cout) stride ldy; D' = D | D/2
// (TF 'same', stride 2) | 2D (transposed).  Cin must be a multiple of 16 and ldx / ldy / the views' first channel multiples of 8.
extern "C" int bts_lp_conv3d_fwd(int kind, int dtype, const void* x, const void* wp, const float* bias, void* y, void* workspace,
                                 long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, hipStream_t stream) {
  if (kind < 0 || kind > 3) return BTS_ERR_UNSUPPORTED;
  return lp_conv_run(kind, dtype, x, wp, bias, y, workspace, workspace_bytes, N, D, H, W, Cin, ldx, Cout, ldy, 0, stream);
}
// y = conv3x3x3(x) + bias in the storage type (dense) AND the slab-mode GroupNorm statistics of y (group_norm.py:83-108 as the
// reference runs it on channels_last data: resnet.py:80-93 conv -> GroupNormalization) in one pass: (sum, sumsq) partials leave the
// conv's epilogue per (z plane, tile column), bts_gn_finalize_partials_ turns them into mean / rstd.  Grids that split the input
// channels, z-slabs that are not whole planes (D % G != 0) and heads with Cout % 4 != 0 run the conv and bts_lp_gn_stats on the stored y.
static long lp_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int G, LpS1Choice& ch) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || G <= 0 || Cout % G != 0) return -1;
  LpS1Call c = lp_s1_call(N, D, H, W, Cin, Cout);
  c.G = G;
  lp_s1_choose(c, ch);
  const long fused = ch.B > 0 ? (long)N * G * ch.B * 16 + 64 : 0;
  const long conv = ((ch.ws + 63) / 64) * 64;
  const long stats = bts_lp_gn_workspace(N, (long)D * H * W, Cout, G);
  return conv + (fused > stats ? fused : stats) + 64;
}
extern "C" long bts_lp_conv3d_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int G) {
  LpS1Choice ch;
  return lp_fwd_gn_workspace(N, D, H, W, Cin, Cout, G, ch);
}
extern "C" int bts_lp_conv3d_fwd_gn(int dtype, const void* x, const void* wp, const float* bias, void* y, float* mean, float* rstd,
                                    void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int G,
                                    float eps, hipStream_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || G <= 0 || Cout % G != 0) return BTS_ERR_SHAPE;
  LpS1Choice sized, ch;
  if (workspace == nullptr || workspace_bytes < lp_fwd_gn_workspace(N, D, H, W, Cin, Cout, G, sized) || (((uintptr_t)workspace) & 15))
    return BTS_ERR_WORKSPACE;
  int r = lp_conv_check(dtype, x, wp, y, N, D, H, W, Cin, ldx, Cout, Cout);
  if (r != BTS_OK) return r;
  LpS1Call c = lp_s1_call(N, D, H, W, Cin, Cout);
  c.ldx = ldx; c.G = G; c.aligned = lp_al16(x) && lp_al16(y) && lp_al16(wp);
  r = lp_s1_choose(c, ch);
  if (r != BTS_OK) return r;
  const long conv_ws = ((sized.ws + 63) / 64) * 64;
  char* tail = reinterpret_cast<char*>(workspace) + conv_ws;
  const long V = (long)D * H * W;
  LpS1Ptrs q{x, wp, bias, y, workspace, conv_ws};
  if (ch.B > 0 && lp_s1_same(ch, sized)) {
    q.gnp = reinterpret_cast<double*>(tail);
    r = lp_s1_run(dtype, c, ch, q, stream);
    if (r != BTS_OK) return r;
    return bts_gn_finalize_partials_(q.gnp, mean, rstd, N * G, ch.B, (double)(V * Cout / G), eps, stream);
  }
  r = lp_s1_run(dtype, c, ch, q, stream);
  if (r != BTS_OK) return r;
  return bts_lp_gn_stats(dtype, y, mean, rstd, tail, workspace_bytes - conv_ws, N, V, Cout, G, BTS_GN_SLAB, eps, stream);
}
// conv1 AND the shortcut of a ResnetBlock from ONE pass over the block input (resnet.py:118 `res = conv3d_ptwise(inputs)` and resnet.py:134
// `x = conv3d_1(inputs)` read the same tensor): y = conv3x3x3(x) + bias with GroupNorm `G`'s statistics of y (as bts_lp_conv3d_fwd_gn), res =
// conv1x1x1(x) + bias_pt and gap[n][c] = mean over the voxels of the unrounded res (as bts_lp_conv1_gap) -- the shortcut is a second set of
// output columns at the centre tap of the z-marching kernel's input planes (lowp_s1z.hip, FS form): x is read once, the 1x1x1 launch and
// its read of x go away.  wp = bts_lp_pack(K3S1, FWD), wp_pt = bts_lp_pack(K1, FWD) with the same Cin_slab / fold; y and res dense
// (N,D,H,W,Cout).  The workspace query returns -1 and the call 1 (nothing launched) where the streaming kernel does not take the shape:
// the caller runs bts_lp_conv1_gap + bts_lp_conv3d_fwd_gn.  BTS_LP_FS=0 in the environment: never (A/B aid).
static long lp_fwd_gn_shortcut_workspace(int N, int D, int H, int W, int Cin, int ldx, int Cout, int G, LpS1Choice& ch) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || G <= 0 || Cout % G != 0) return -1;
  LpS1Call c = lp_s1_call(N, D, H, W, Cin, Cout);
  // (a voxel stride below Cin: the two 32-channel halves are dense tensors of their own -- the two-pass form)
  c.ldx = ldx; c.ldxb = ldx < Cin ? ldx : 0; c.G = G; c.Cout2 = c.ldy2 = Cout;
  if (lp_s1_choose(c, ch) != BTS_OK || ch.B <= 0) return -1;
  return (long)N * G * ch.B * 16 + 64 + (long)N * lp_s1z_fs_B(ch.z) * Cout * 8 + 64;
}
extern "C" long bts_lp_conv3d_fwd_gn_shortcut_workspace(int N, int D, int H, int W, int Cin, int ldx, int Cout, int G) {
  LpS1Choice ch;
  return lp_fwd_gn_shortcut_workspace(N, D, H, W, Cin, ldx, Cout, G, ch);
}
extern "C" int bts_lp_conv3d_fwd_gn_shortcut(int dtype, const void* x, long x_split, const void* wp, const float* bias, void* y, float* mean,
                                             float* rstd, const void* wp_pt, const float* bias_pt, void* res, float* gap, void* workspace,
                                             long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int G, float eps,
                                             hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  LpS1Choice sized, ch;
  const long need = lp_fwd_gn_shortcut_workspace(N, D, H, W, Cin, ldx, Cout, G, sized);
  if (need < 0) return 1;
  if (workspace == nullptr || workspace_bytes < need || (((uintptr_t)workspace) & 15)) return BTS_ERR_WORKSPACE;
  if (x == nullptr || wp == nullptr || wp_pt == nullptr || y == nullptr || res == nullptr || gap == nullptr || mean == nullptr || rstd == nullptr)
    return BTS_ERR_ALIGN;
  if (ldx % 8 != 0 || ldx < (x_split ? 32 : Cin) || !lp_al16(x) || !lp_al16(wp)) return BTS_ERR_ALIGN;
  if (x_split != 0 && (Cin != 64 || x_split < 0 || x_split % 8 != 0)) return BTS_ERR_SHAPE;      // (two 32-channel operands: the two-pass form)
  const void* xb = x_split ? static_cast<const void*>(reinterpret_cast<const unsigned short*>(x) + x_split) : nullptr;
  LpS1Call c = lp_s1_call(N, D, H, W, Cin, Cout);
  c.ldx = ldx; c.ldxb = x_split ? ldx : 0; c.G = G; c.Cout2 = c.ldy2 = Cout;
  c.aligned = lp_al16(x) && lp_al16(y) && lp_al16(wp) && lp_al16(wp_pt) && lp_al16(res) && lp_al16(xb);
  if (lp_s1_choose(c, ch) != BTS_OK || !lp_s1_same(ch, sized)) return 1;
  const long Bg = ch.B, Bf = lp_s1z_fs_B(ch.z);
  LpS1Ptrs q{x, wp, bias, y};
  q.gnp = reinterpret_cast<double*>(workspace);
  q.wp2 = wp_pt; q.y2 = res; q.bias2 = bias_pt; q.xb = xb;
  q.gap_part = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + (((long)N * G * Bg * 16 + 63) / 64) * 64);
  const long V = (long)D * H * W;
  const int r = lp_s1_run(dtype, c, ch, q, stream);
  if (r != BTS_OK) return r;
  const int r2 = bts_gn_finalize_partials_(q.gnp, mean, rstd, N * G, Bg, (double)(V * Cout / G), eps, stream);
  if (r2 != BTS_OK) return r2;
  return bts_lp_colsum_finalize_(q.gap_part, gap, N, Cout, (int)Bf, 1.0 / (double)V, stream);
}
// The same with GroupNorm + ReLU of the INPUT applied on the way in (in_relu must be 1): y = conv3x3x3(relu(GN_in(x))) + bias and the statistics of y --
// conv2 of a ResnetBlock reading conv1's raw output (resnet.py:133-136: conv -> GroupNormalization -> relu -> conv) where no backward
// needs the normalised tensor (inference, test.py:128-151 via Model.call(inference=True)).  The workspace query returns -1 where the
// streaming kernel does not take the shape in this form (the caller runs bts_lp_gn_apply + bts_lp_conv3d_fwd_gn).
static long lp_gnin_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int in_G, int G, LpS1Choice& ch) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || G <= 0 || Cout % G != 0 || in_G <= 0 || Cin % in_G != 0) return -1;
  LpS1Call c = lp_s1_call(N, D, H, W, Cin, Cout);
  c.G = G; c.gna_G = in_G;
  if (lp_s1_choose(c, ch) != BTS_OK || ch.B <= 0) return -1;
  return (long)N * G * ch.B * 16 + 128;
}
extern "C" long bts_lp_conv3d_gnin_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int in_G, int G) {
  LpS1Choice ch;
  return lp_gnin_fwd_gn_workspace(N, D, H, W, Cin, Cout, in_G, G, ch);
}
extern "C" int bts_lp_conv3d_gnin_fwd_gn(int dtype, const void* x, const float* in_gamma, const float* in_beta, const float* in_mean,
                                         const float* in_rstd, int in_G, int in_relu, const void* wp, const float* bias, void* y, float* mean,
                                         float* rstd, void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int Cout, int G,
                                         float eps, hipStream_t stream) {
  LpS1Choice sized, ch;
  const long need = lp_gnin_fwd_gn_workspace(N, D, H, W, Cin, Cout, in_G, G, sized);
  if (need < 0 || !in_relu) return BTS_ERR_UNSUPPORTED;      // (the kernel form that exists applies GroupNorm + ReLU)
  if (workspace == nullptr || workspace_bytes < need || (((uintptr_t)workspace) & 15)) return BTS_ERR_WORKSPACE;
  const int chk = lp_conv_check(dtype, x, wp, y, N, D, H, W, Cin, Cin, Cout, Cout);
  if (chk != BTS_OK) return chk;
  LpS1Call c = lp_s1_call(N, D, H, W, Cin, Cout);
  c.G = G; c.gna_G = in_G; c.aligned = lp_al16(x) && lp_al16(y) && lp_al16(wp);
  if (lp_s1_choose(c, ch) != BTS_OK || !lp_s1_same(ch, sized)) return BTS_ERR_UNSUPPORTED;
  const LpGnaFuse ga{in_gamma, in_beta, in_mean, in_rstd, in_G, Cin / in_G};
  LpS1Ptrs q{x, wp, bias, y};
  q.gnp = reinterpret_cast<double*>(workspace); q.ga = &ga;
  const int r = lp_s1_run(dtype, c, ch, q, stream);
  if (r != BTS_OK) return r;
  return bts_gn_finalize_partials_(q.gnp, mean, rstd, N * G, ch.B, (double)((long)D * H * W * Cout / G), eps, stream);
}
// dx (+)= conv^T(dy) (replaces tf.GradientTape for these ops, train.py:142-151).  (D,H,W) are the forward INPUT dims, Cin / Cout
// the forward channel counts; wp_bwd = bts_lp_pack(kind, BTS_ROLE_BWD_DATA, ...).  The data gradient of each kind is one of the
// forward geometries on the role-swapped image: stride 1 -> stride 1 with flipped taps, 1x1x1 -> 1x1x1, stride 2 -> the
// transposed form's parity classes (each input voxel receives from (o, k=i-2o)), transposed -> the stride-2 gather.
extern "C" long bts_lp_conv3d_bwd_data_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  return kind == BTS_CONV_K3S1 ? lp_s1_workspace(N, D, H, W, Cout, Cin) : 0;
}
extern "C" int bts_lp_conv3d_bwd_data(int kind, int dtype, const void* dy, const void* wp_bwd, void* dx, void* workspace,
                                      long workspace_bytes, int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy, int accum,
                                      hipStream_t stream) {
  switch (kind) {
    case BTS_CONV_K1:
    case BTS_CONV_K3S1:
      return lp_conv_run(kind, dtype, dy, wp_bwd, nullptr, dx, workspace, workspace_bytes, N, D, H, W, Cout, lddy, Cin, lddx, accum, stream);
    case BTS_CONV_K3S2:   // dy lives on the half grid; TF 'same' with even sizes pads (0,1) only, which is what the class tables assume
      if ((D | H | W) & 1) return BTS_ERR_UNSUPPORTED;
      return lp_conv_run(3, dtype, dy, wp_bwd, nullptr, dx, workspace, workspace_bytes, N, D / 2, H / 2, W / 2, Cout, lddy, Cin, lddx, accum, stream);
    case BTS_CONV_K3S2T:  // dy lives on the doubled grid: dx[i] = sum_k dy[2i+k] W[k]
      return lp_conv_run(2, dtype, dy, wp_bwd, nullptr, dx, workspace, workspace_bytes, N, 2 * D, 2 * H, 2 * W, Cout, lddy, Cin, lddx, accum, stream);
  }
  return BTS_ERR_UNSUPPORTED;
}
// dx (+)= conv3x3x3^T(dy) + conv1x1x1^T(dy2) in ONE launch: the data gradients of the two convolutions that read a ResnetBlock's input
// (resnet.py:80-87 conv1 and resnet.py:96-103 the shortcut, both applied to `inputs`: resnet.py:118,134) meet in dx under train.py:151.
// The shortcut's contraction rides on conv1's as an extra K-segment at the CENTRE tap (K more matrix steps per 27 K: 3.7 %), its operand
// dy2 read straight from global memory into the matrix instruction -- instead of a second launch that read-modify-writes the Cin-wide dx.
// dy, dy2: (N,D,H,W,Cout) with voxel strides lddy / lddy2; wp_bwd / wp2_bwd: bts_lp_pack(K3S1 / K1, BTS_ROLE_BWD_DATA, ...) of the two
// kernels with the same Cin_slab / fold.  Shapes the fused kernels do not take run as the two launches they replace (same result up to the
// one extra rounding of the stored intermediate): the call always completes.  *fused (may be NULL): 1 if the one-launch form ran.
// dx_split (elements; 0 = dx is one (N,D,H,W,Cin) view): columns [32 b, 32 b + 32) of the result go to dx + b * dx_split, each block a
// tensor of its own with voxel stride lddx -- the gradient of a concat of 32-channel tensors (decoder.py:75) leaves as dense tensors whose
// readers fetch whole lines.  Only the fused tiled kernel writes that form: ask bts_lp_conv3d_bwd_data_sc_split_ok first.
// (role-swapped: the contraction runs over the forward's Cout, the columns are the forward's Cin; the query's view: dense dy, dy2, dx)
static LpS1Call lp_sc_call(int N, int D, int H, int W, int Cin, int Cout, long dx_split) {
  LpS1Call c = lp_s1_call(N, D, H, W, Cout, Cin);
  c.ldx2 = Cout; c.ysplit = dx_split;
  if (dx_split != 0) c.ldy = 32;
  return c;
}
extern "C" long bts_lp_conv3d_bwd_data_sc_workspace(int N, int D, int H, int W, int Cin, int Cout) {
  LpS1Choice ch;
  return lp_s1_choose(lp_sc_call(N, D, H, W, Cin, Cout, 0), ch) >= 0 ? ch.ws : 0;      // (1: the two launches' K3S1 conv)
}
extern "C" int bts_lp_conv3d_bwd_data_sc_split_ok(int N, int D, int H, int W, int Cin, int Cout) {
  LpS1Choice ch;
  return lp_s1_choose(lp_sc_call(N, D, H, W, Cin, Cout, (long)N * D * H * W * 32), ch) == BTS_OK ? 1 : 0;
}
extern "C" int bts_lp_conv3d_bwd_data_sc(int dtype, const void* dy, const void* wp_bwd, const void* dy2, const void* wp2_bwd, void* dx,
                                         long dx_split, void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int lddx,
                                         int Cout, int lddy, int lddy2, int accum, int* fused, hipStream_t stream) {
  if (fused) *fused = 0;
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return BTS_ERR_SHAPE;
  if (dy == nullptr || dy2 == nullptr || wp_bwd == nullptr || wp2_bwd == nullptr || dx == nullptr) return BTS_ERR_ALIGN;
  LpS1Choice sized, ch;
  lp_s1_choose(lp_sc_call(N, D, H, W, Cin, Cout, dx_split), sized);
  LpS1Call c = lp_sc_call(N, D, H, W, Cin, Cout, dx_split);
  c.ldx = lddy; c.ldx2 = lddy2; c.ldy = lddx; c.accum = accum;
  c.aligned = lp_al16(dy) && lp_al16(dy2) && lp_al16(dx) && lp_al16(wp_bwd) && lp_al16(wp2_bwd) && dx_split % 8 == 0;
  if (lp_s1_choose(c, ch) == BTS_OK && lp_s1_same(ch, sized)) {
    LpS1Ptrs q{dy, wp_bwd, nullptr, dx, workspace, workspace_bytes};
    q.x2 = dy2; q.wp2 = wp2_bwd;
    const int r = lp_s1_run(dtype, c, ch, q, stream);
    if (r == BTS_OK && fused) *fused = 1;
    return r;
  }
  if (dx_split != 0) return BTS_ERR_UNSUPPORTED;      // (the two-launch route writes one tensor)
  const int r = lp_conv_run(1, dtype, dy, wp_bwd, nullptr, dx, workspace, workspace_bytes, N, D, H, W, Cout, lddy, Cin, lddx, accum, stream);
  if (r != BTS_OK) return r;
  return lp_conv_run(0, dtype, dy2, wp2_bwd, nullptr, dx, nullptr, 0, N, D, H, W, Cout, lddy2, Cin, lddx, 1, stream);
}
