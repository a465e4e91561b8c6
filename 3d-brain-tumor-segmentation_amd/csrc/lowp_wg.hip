// 16-bit weight gradients: the general LDS-tiled kernel, the fixed-order finalize every weight-gradient kernel shares, and the host side of
// all of them -- lp_wg_choose (which kernel takes a call and where its workspace areas lie: lowp_common.h), the workspace queries and the
// entry points.  The streaming kernel lives in lowp_wgd.hip, the strided one in lowp_wgs.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.h"
#include "bts_internal.h"
#include "lowp_common.h"

// =====================================================================================================================
// Weight gradient of the stride-1 3x3x3 and 1x1x1 convolutions on 16-bit operands (what TF autodiff derives for the Conv3D
// kernels of resnet.py:30-37,80-87,96-103; train.py:151):  dW[t][c][k] = sum_v P[v + off_t][c] * Q[v][k],  P = the conv's input,
// Q = the gradient of its output.  The contraction runs over VOXELS, so both matrix operands want 8 consecutive voxels of one
// channel per lane (v_mfma_f32_32x32x16: A row = input channel, B column = output channel, K = 16 voxels along x) while memory is
// channel-fastest: the (halo) tiles are staged voxel-major in LDS as they come and every fragment is gathered with eight
// 2-byte LDS reads -- taps, which shift the 8-voxel window by single voxels, cost nothing extra that way.  A Q fragment serves all
// of a wave's taps, a P fragment all of its cout blocks.  8 waves: the 27 taps are dealt round-robin (1x1x1: the 32 x-rows of the
// tile are), persistent workgroups accumulate over their tiles and leave fp32 partials for a fixed-order finalize that also folds
// the encoder's duplicated slice back onto both copies of the weight (encoder.py:83-87) and adds into the gradient buffer.
// =====================================================================================================================
struct LpWgParams {
  const unsigned short* p;
  const unsigned short* q;
  float* part;
  int N, D, H, W, Cp, ldp, Cq, ldq, ntaps;
  int ntx, nty, ntz;
  long ntiles;
  int ncp, ncqg;
};
#define LPW_TX 16
#define LPW_TY 8
#define LPW_TZ 4

template <typename T, int NQ, bool K3>
__global__ __launch_bounds__(512, 1) void lp_wgrad_kernel(const LpWgParams p) {
  constexpr int TX = LPW_TX, TY = LPW_TY, TZ = LPW_TZ;
  constexpr int PS = 36, QS = 32 * NQ + 4;          // halves per staged voxel (8-byte aligned rows, bank-skewed)
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  constexpr bool k3 = K3;
  constexpr int halo = K3 ? 1 : 0;
  constexpr int SX = TX + 2 * halo, SY = TY + 2 * halo, SZ = TZ + 2 * halo;
  constexpr int nvp = SX * SY * SZ;
  unsigned short* ldsP = lds;
  unsigned short* ldsQ = lds + (TX + 2) * (TY + 2) * (TZ + 2) * PS;
  const int cpt = blockIdx.y / p.ncqg, cqg = blockIdx.y % p.ncqg;
  const int cp0 = cpt * 32, cq0 = cqg * 32 * NQ;
  f32x16 acc[4][NQ];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int c = 0; c < NQ; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][c][r] = 0.f;
  auto tile_origin = [&](long tile, int& n, int& x0, int& y0, int& z0) {
    long b = tile;
    const int tx = (int)(b % p.ntx); b /= p.ntx;
    const int ty = (int)(b % p.nty); b /= p.nty;
    const int tz = (int)(b % p.ntz);
    n = (int)(b / p.ntz);
    x0 = tx * TX; y0 = ty * TY; z0 = tz * TZ;
  };

  if constexpr (K3) {
    // ---- 3x3x3: LDS tiles with PAIRS of x-neighbours interleaved per channel, [row (z, y)][x pair][channel] dwords (low half = the
    // even slot).  A matrix operand (8 consecutive voxels of one channel) is then 4 consecutive pair-dwords of a lane's channel: 4 or
    // 5 ds_read_b32 + 4 v_alignbit (a tap's window starts at an odd slot for kx = 0, 2) instead of eight 2-byte reads and their
    // packing.  Staging interleaves two voxels' 8-channel chunks with v_perm and writes 32 contiguous bytes.
    constexpr int NPP = (SX + 2) / 2;            // pairs per P row: slots x = -2 .. SX - 1
    constexpr int NPQ = TX / 2;
    constexpr int PU = SZ * SY * NPP * 4, QU = TZ * TY * NPQ * 4 * NQ;    // staging units: (row, pair, channel octet)
    constexpr int PUS = (PU + 511) / 512, QUS = (QU + 511) / 512;
    unsigned* const ldsP32 = reinterpret_cast<unsigned*>(lds);
    unsigned* const ldsQ32 = ldsP32 + SZ * SY * NPP * 32;
    u32x4 preP[PUS][2], preQ[QUS][2];
    auto fetch = [&](long tile) {
      int n, x0, y0, z0;
      tile_origin(tile, n, x0, y0, z0);
#pragma unroll
      for (int i = 0; i < PUS; ++i) {
        const int e = tid + i * 512;
        preP[i][0] = preP[i][1] = u32x4{0u, 0u, 0u, 0u};
        if (e < PU) {
          const int oct = e & 3, xp = (e >> 2) % NPP, row = (e >> 2) / NPP;
          const int gz = z0 - 1 + row / SY, gy = y0 - 1 + row % SY;
          if ((unsigned)gz < (unsigned)p.D && (unsigned)gy < (unsigned)p.H && cp0 + oct * 8 < p.Cp) {
            const unsigned short* rowp = p.p + (((long)n * p.D + gz) * p.H + gy) * (long)p.W * p.ldp + cp0 + oct * 8;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const int slot = 2 * xp + s2, gx = x0 - 2 + slot;   // slots 1 .. SX are the halo tile's columns -1 .. TX
              if (slot >= 1 && slot <= SX && (unsigned)gx < (unsigned)p.W) preP[i][s2] = *reinterpret_cast<const u32x4*>(rowp + (long)gx * p.ldp);
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < QUS; ++i) {
        const int e = tid + i * 512;
        preQ[i][0] = preQ[i][1] = u32x4{0u, 0u, 0u, 0u};
        if (e < QU) {
          const int oct = e % (4 * NQ), xp = (e / (4 * NQ)) % NPQ, row = e / (4 * NQ * NPQ);
          const int gz = z0 + row / TY, gy = y0 + row % TY;
          if (gz < p.D && gy < p.H && cq0 + oct * 8 < p.Cq) {
            const unsigned short* rowq = p.q + (((long)n * p.D + gz) * p.H + gy) * (long)p.W * p.ldq + cq0 + oct * 8;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const int gx = x0 + 2 * xp + s2;
              if (gx < p.W) preQ[i][s2] = *reinterpret_cast<const u32x4*>(rowq + (long)gx * p.ldq);
            }
          }
        }
      }
    };
    // (even voxel's channels c, c+1 | odd voxel's c, c+1) x 4 -> channel c: (even, odd), channel c+1: (even, odd)
    auto weave = [&](const u32x4 ev, const u32x4 od, unsigned* dst) {
      u32x4 lo, hi;
      lo[0] = __builtin_amdgcn_perm(od[0], ev[0], 0x05040100u); lo[1] = __builtin_amdgcn_perm(od[0], ev[0], 0x07060302u);
      lo[2] = __builtin_amdgcn_perm(od[1], ev[1], 0x05040100u); lo[3] = __builtin_amdgcn_perm(od[1], ev[1], 0x07060302u);
      hi[0] = __builtin_amdgcn_perm(od[2], ev[2], 0x05040100u); hi[1] = __builtin_amdgcn_perm(od[2], ev[2], 0x07060302u);
      hi[2] = __builtin_amdgcn_perm(od[3], ev[3], 0x05040100u); hi[3] = __builtin_amdgcn_perm(od[3], ev[3], 0x07060302u);
      reinterpret_cast<u32x4*>(dst)[0] = lo;
      reinterpret_cast<u32x4*>(dst)[1] = hi;
    };
    auto commit = [&]() {
#pragma unroll
      for (int i = 0; i < PUS; ++i) {
        const int e = tid + i * 512;
        if (e < PU) weave(preP[i][0], preP[i][1], ldsP32 + (e >> 2) * 32 + (e & 3) * 8);
      }
#pragma unroll
      for (int i = 0; i < QUS; ++i) {
        const int e = tid + i * 512;
        if (e < QU) weave(preQ[i][0], preQ[i][1], ldsQ32 + (e / (4 * NQ)) * (32 * NQ) + (e % (4 * NQ)) * 8);
      }
    };
    if constexpr (NQ == 1) {
      // Tap dealing: six compute waves = (dy, half of the tile's y rows); a wave walks the P rows (z', y' = y + dy) of its four y
      // and uses each row's three x windows (kx = 0, 1, 2: window starts at slots 1, 2, 3 -- six pair reads, five alignbits) for
      // ALL three dz with the Q rows z = z' - dz, which roll through three fragment registers: 10 LDS reads + 5 vector-ALU
      // instructions per 9 matrix instructions at full depth.  Nine accumulators (dz, kx) per wave; the two halves of a dy meet in
      // LDS at the end.  Waves 6, 7 only help staging.
      const bool cw = wave < 6;
      const int dy = wave % 3, half = (wave / 3) & 1;
      const unsigned* pbase = ldsP32 + 4 * h * 32 + l32;
      const unsigned* qbase = ldsQ32 + 4 * h * 32 + l32;
      f32x16 a9[3][3];
  #pragma unroll
      for (int dz = 0; dz < 3; ++dz)
  #pragma unroll
        for (int kx = 0; kx < 3; ++kx)
  #pragma unroll
          for (int r = 0; r < 16; ++r) a9[dz][kx][r] = 0.f;
      long tile = blockIdx.x;
      if (tile < p.ntiles) fetch(tile);
      for (; tile < p.ntiles; tile += gridDim.x) {
        __syncthreads();      // every wave is done with the previous tile
        commit();
        __syncthreads();
        if (tile + gridDim.x < p.ntiles) fetch(tile + gridDim.x);
        if (cw) {
  #pragma unroll 2
          for (int yi = 0; yi < TY / 2; ++yi) {
            const int yq = half * (TY / 2) + yi;
            const unsigned* prow = pbase + ((yq + dy) * NPP) * 32;
            const unsigned* qrow = qbase + (yq * NPQ) * 32;
            u32x4 qf[3];
  #pragma unroll
            for (int zp = 0; zp < SZ; ++zp) {
              if (zp < TZ) {
                const unsigned* qr = qrow + (zp * TY * NPQ) * 32;
                qf[zp % 3] = u32x4{qr[0], qr[32], qr[64], qr[96]};
              }
              const unsigned* pr = prow + (zp * SY * NPP) * 32;
              unsigned pp[6], sh[5];
  #pragma unroll
              for (int k = 0; k < 6; ++k) pp[k] = pr[k * 32];
  #pragma unroll
              for (int k = 0; k < 5; ++k) sh[k] = __builtin_amdgcn_alignbit(pp[k + 1], pp[k], 16);
              const u32x4 w0 = {sh[0], sh[1], sh[2], sh[3]}, w1 = {pp[1], pp[2], pp[3], pp[4]}, w2 = {sh[1], sh[2], sh[3], sh[4]};
  #pragma unroll
              for (int dz = 0; dz < 3; ++dz) {
                const int z = zp - dz;
                if (z >= 0 && z < TZ) {
                  a9[dz][0] = T::mfma(w0, qf[z % 3], a9[dz][0]);
                  a9[dz][1] = T::mfma(w1, qf[z % 3], a9[dz][1]);
                  a9[dz][2] = T::mfma(w2, qf[z % 3], a9[dz][2]);
                }
              }
            }
          }
        }
      }
      // the two halves of a dy: waves 3..5 hand their nine accumulators over through LDS, waves 0..2 add and write the partials
      __syncthreads();
      float* xch = reinterpret_cast<float*>(lds);
      if (wave >= 3 && wave < 6) {
  #pragma unroll
        for (int dz = 0; dz < 3; ++dz)
  #pragma unroll
          for (int kx = 0; kx < 3; ++kx)
  #pragma unroll
            for (int r = 0; r < 16; ++r) xch[((((wave - 3) * 9 + dz * 3 + kx) * 16) + r) * 64 + lane] = a9[dz][kx][r];
      }
      __syncthreads();
      if (wave < 3) {
        float* pb = p.part + (((long)blockIdx.x * p.ncp + cpt) * p.ncqg + cqg) * (long)27 * 32 * 32;
  #pragma unroll
        for (int dz = 0; dz < 3; ++dz)
  #pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int slot = (dz * 3 + dy) * 3 + kx;
  #pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
              pb[((long)slot * 32 + row) * 32 + l32] = a9[dz][kx][r] + xch[(((wave * 9 + dz * 3 + kx) * 16) + r) * 64 + lane];
            }
          }
      }
      return;
    } else {
      // wave w owns taps w, w+8, w+16 (and w+24 for w < 3) and walks all 32 x-rows of the tile; a tap's window starts at slot
      // kx + 1 (+ 8 for the lanes of the upper K half): pair offset and alignbit shift are wave constants
      int toff[4], tsh[4];
  #pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        const int t = wave + 8 * ti;
        const int tt = t < 27 ? t : 0;
        const int kx = tt % 3;
        toff[ti] = ((((tt / 9) * SY + (tt / 3) % 3) * NPP) + ((kx + 1) >> 1)) * 32;
        tsh[ti] = ((kx + 1) & 1) ? 16 : 0;
      }
      const bool t3 = wave + 24 < 27;
      const unsigned* pbase = ldsP32 + 4 * h * 32 + l32;
      const unsigned* qbase = ldsQ32 + 4 * h * (32 * NQ) + l32;
      auto pfrag = [&](const unsigned* prow, int off, int sh) {
        unsigned pp[5];
  #pragma unroll
        for (int k = 0; k < 5; ++k) pp[k] = prow[off + k * 32];
        return u32x4{__builtin_amdgcn_alignbit(pp[1], pp[0], sh), __builtin_amdgcn_alignbit(pp[2], pp[1], sh),
                     __builtin_amdgcn_alignbit(pp[3], pp[2], sh), __builtin_amdgcn_alignbit(pp[4], pp[3], sh)};
      };
      long tile = blockIdx.x;
      if (tile < p.ntiles) fetch(tile);
      for (; tile < p.ntiles; tile += gridDim.x) {
        __syncthreads();      // every wave is done with the previous tile
        commit();
        __syncthreads();
        if (tile + gridDim.x < p.ntiles) fetch(tile + gridDim.x);
  #pragma unroll 4
        for (int kb = 0; kb < TY * TZ; ++kb) {
          const int z = kb / TY, y = kb % TY;
          u32x4 bq[NQ];
  #pragma unroll
          for (int c = 0; c < NQ; ++c) {
            const unsigned* qr = qbase + (kb * NPQ) * (32 * NQ) + c * 32;
            bq[c] = u32x4{qr[0], qr[32 * NQ], qr[2 * 32 * NQ], qr[3 * 32 * NQ]};
          }
          const unsigned* prow = pbase + ((z * SY + y) * NPP) * 32;
  #pragma unroll
          for (int ti = 0; ti < 3; ++ti) {
            const u32x4 a = pfrag(prow, toff[ti], tsh[ti]);
  #pragma unroll
            for (int c = 0; c < NQ; ++c) acc[ti][c] = T::mfma(a, bq[c], acc[ti][c]);
          }
          if (t3) {
            const u32x4 a = pfrag(prow, toff[3], tsh[3]);
  #pragma unroll
            for (int c = 0; c < NQ; ++c) acc[3][c] = T::mfma(a, bq[c], acc[3][c]);
          }
        }
      }
    }
  } else {
    // ---- 1x1x1: voxel-major tiles as they come, every fragment gathered with eight 2-byte LDS reads; wave w takes x-rows w, w+8,
    // w+16, w+24 (one accumulator per wave; the finalize adds the eight)
    constexpr int PSLOT = (nvp * 4 + 511) / 512;   // 16-byte chunks of the P tile per thread
    constexpr int QSLOT = (TX * TY * TZ * 4 * NQ + 511) / 512;
    u32x4 preP[PSLOT], preQ[QSLOT];
    auto fetch = [&](long tile) {
      int n, x0, y0, z0;
      tile_origin(tile, n, x0, y0, z0);
#pragma unroll
      for (int i = 0; i < PSLOT; ++i) {
        const int e = tid + i * 512;
        preP[i] = u32x4{0u, 0u, 0u, 0u};
        if (e < nvp * 4) {
          const int vox = e >> 2, cq = e & 3;
          const int vz = vox / (SY * SX), r = vox - vz * (SY * SX), vy = r / SX, vx = r - vy * SX;
          const int gz = z0 - halo + vz, gy = y0 - halo + vy, gx = x0 - halo + vx;
          if ((unsigned)gz < (unsigned)p.D && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W && cp0 + cq * 8 < p.Cp)
            preP[i] = *reinterpret_cast<const u32x4*>(p.p + ((((long)n * p.D + gz) * p.H + gy) * p.W + gx) * (long)p.ldp + cp0 + cq * 8);
        }
      }
#pragma unroll
      for (int i = 0; i < QSLOT; ++i) {
        const int e = tid + i * 512;
        preQ[i] = u32x4{0u, 0u, 0u, 0u};
        if (e < TX * TY * TZ * 4 * NQ) {
          const int vox = e / (4 * NQ), cq = e % (4 * NQ);
          const int vz = vox / (TY * TX), r = vox - vz * (TY * TX), vy = r / TX, vx = r - vy * TX;
          const int gz = z0 + vz, gy = y0 + vy, gx = x0 + vx;
          if (gz < p.D && gy < p.H && gx < p.W && cq0 + cq * 8 < p.Cq)
            preQ[i] = *reinterpret_cast<const u32x4*>(p.q + ((((long)n * p.D + gz) * p.H + gy) * p.W + gx) * (long)p.ldq + cq0 + cq * 8);
        }
      }
    };
    auto commit = [&]() {
#pragma unroll
      for (int i = 0; i < PSLOT; ++i) {
        const int e = tid + i * 512;
        if (e < nvp * 4) {
          u32x2* d = reinterpret_cast<u32x2*>(ldsP + (e >> 2) * PS + (e & 3) * 8);
          d[0] = u32x2{preP[i][0], preP[i][1]};
          d[1] = u32x2{preP[i][2], preP[i][3]};
        }
      }
#pragma unroll
      for (int i = 0; i < QSLOT; ++i) {
        const int e = tid + i * 512;
        if (e < TX * TY * TZ * 4 * NQ) {
          u32x2* d = reinterpret_cast<u32x2*>(ldsQ + (e / (4 * NQ)) * QS + (e % (4 * NQ)) * 8);
          d[0] = u32x2{preQ[i][0], preQ[i][1]};
          d[1] = u32x2{preQ[i][2], preQ[i][3]};
        }
      }
    };
    // eight 2-byte reads -> one 16-byte matrix operand (K = 8 consecutive voxels along x of one channel)
    auto gather = [&](const unsigned short* base, int stride) {
      unsigned v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = base[j * stride];
      return u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
    };
    long tile = blockIdx.x;
    if (tile < p.ntiles) fetch(tile);
    for (; tile < p.ntiles; tile += gridDim.x) {
      __syncthreads();      // every wave is done with the previous tile
      commit();
      __syncthreads();
      if (tile + gridDim.x < p.ntiles) fetch(tile + gridDim.x);
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        const int kb = wave + 8 * ti;
        const int z = kb / TY, y = kb % TY;
        const u32x4 a = gather(ldsP + ((z * SY + y) * SX + 8 * h) * PS + l32, PS);
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          const u32x4 b = gather(ldsQ + ((z * TY + y) * TX + 8 * h) * QS + c * 32 + l32, QS);
          acc[0][c] = T::mfma(a, b, acc[0][c]);
        }
      }
    }
  }
  // partial sums: part[wg][cp tile][cq group][slot][32 cin][32*NQ cout]; slot = tap (3x3x3) or wave (1x1x1)
  const int nslot = k3 ? 27 : 8;
  float* pb = p.part + (((long)blockIdx.x * p.ncp + cpt) * p.ncqg + cqg) * (long)nslot * 32 * (32 * NQ);
#pragma unroll
  for (int ti = 0; ti < 4; ++ti) {
    const int slot = k3 ? wave + 8 * ti : wave;
    if ((k3 && slot < 27) || (!k3 && ti == 0)) {
#pragma unroll
      for (int c = 0; c < NQ; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
          pb[((long)slot * 32 + row) * (32 * NQ) + c * 32 + l32] = acc[ti][c][r];
        }
    }
  }
}

struct LpWfParams {
  const float* part;
  float* dw;
  int nwg, ncp, ncqg, nslot, ntaps, NQ, Cp, Cq, Cin_ref, dup_start, dup_shift, accum;
};
// dW[t][c_ref][k] (+)= sum over workgroups (and, for 1x1x1, waves) of the partials, fixed order; a slab channel c is reference
// channel c + shift and, inside the duplicated slice, ALSO reference channel c - dup_start (both copies get the gradient)
__global__ __launch_bounds__(256) void lp_wgrad_finalize_kernel(const LpWfParams f) {
  // 32 consecutive elements x 8 slices of the workgroup list per block: coalesced partial reads, slices combined in fixed order
  __shared__ double sh[8][32];
  const long total = (long)f.ntaps * f.Cp * f.Cq;
  const int el = threadIdx.x & 31, sl = threadIdx.x >> 5;
  for (long i0 = blockIdx.x * 32L; i0 < total; i0 += (long)gridDim.x * 32) {
    const long i = i0 + el;
    double s = 0.0;
    int k = 0, c = 0, t = 0;
    if (i < total) {
      k = (int)(i % f.Cq);
      const long r = i / f.Cq;
      c = (int)(r % f.Cp);
      t = (int)(r / f.Cp);
      const int cpt = c / 32, row = c % 32, cqg = k / (32 * f.NQ), col = k % (32 * f.NQ);
      const int s0 = f.ntaps == 27 ? t : 0, s1 = f.ntaps == 27 ? t + 1 : f.nslot;      // (1x1x1: the general kernel's 8 wave slots, the streaming kernel's one)
      for (int wg = sl; wg < f.nwg; wg += 8) {
        const float* pb = f.part + (((long)wg * f.ncp + cpt) * f.ncqg + cqg) * (long)f.nslot * 32 * (32 * f.NQ);
        for (int q = s0; q < s1; ++q) s += pb[((long)q * 32 + row) * (32 * f.NQ) + col];
      }
    }
    __syncthreads();
    sh[sl][el] = s;
    __syncthreads();
    if (sl == 0 && i < total) {
      double tot = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) tot += sh[q][el];
      const float v = (float)tot;
      float* d0 = f.dw + ((long)t * f.Cin_ref + c + f.dup_shift) * f.Cq + k;
      *d0 = f.accum ? *d0 + v : v;
      if (f.dup_shift > 0 && c >= f.dup_start && c < f.dup_start + f.dup_shift) {
        float* d1 = f.dw + ((long)t * f.Cin_ref + (c - f.dup_start)) * f.Cq + k;
        *d1 = f.accum ? *d1 + v : v;
      }
    }
  }
}
// The same for the 3x3x3 launches (one slot per tap) with Cq % 4 == 0: a thread owns FOUR consecutive columns (16-byte partial reads:
// the 4-byte version above read 28 MB in 29 us = 1 TB/s, 1.7 ms of the batch-8 step), 32 threads x 4 = 128 elements x 8 slices per block
__global__ __launch_bounds__(256) void lp_wgrad_finalize4_kernel(const LpWfParams f) {
  __shared__ double sh[8][32][4];
  const long total4 = (long)f.ntaps * f.Cp * f.Cq / 4;
  const int el = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int W = 32 * f.NQ;
  for (long i0 = blockIdx.x * 32L; i0 < total4; i0 += (long)gridDim.x * 32) {
    const long i4 = i0 + el;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int k = 0, c = 0, t = 0;
    if (i4 < total4) {
      const long i = i4 * 4;
      k = (int)(i % f.Cq);
      const long r = i / f.Cq;
      c = (int)(r % f.Cp);
      t = (int)(r / f.Cp);
      const int cpt = c / 32, row = c % 32, cqg = k / W, col = k % W;
      for (int wg = sl; wg < f.nwg; wg += 8) {
        const float* pb = f.part + (((long)wg * f.ncp + cpt) * f.ncqg + cqg) * (long)f.nslot * 32 * W;
        const f32x4 v = *reinterpret_cast<const f32x4*>(pb + ((long)t * 32 + row) * W + col);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[sl][el][j] = s[j];
    __syncthreads();
    if (sl == 0 && i4 < total4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) tot += sh[q][el][j];
        const float v = (float)tot;
        float* d0 = f.dw + ((long)t * f.Cin_ref + c + f.dup_shift) * f.Cq + k + j;
        *d0 = f.accum ? *d0 + v : v;
        if (f.dup_shift > 0 && c >= f.dup_start && c < f.dup_start + f.dup_shift) {
          float* d1 = f.dw + ((long)t * f.Cin_ref + (c - f.dup_start)) * f.Cq + k + j;
          *d1 = f.accum ? *d1 + v : v;
        }
      }
    }
  }
}
int bts_lp_wgrad_finalize_(const float* part, float* dw, int nwg, int ncp, int ncqg, int nslot, int ntaps, int NQ, int Cp, int Cq, int Cin_ref,
                           int dup_start, int dup_shift, int accum, hipStream_t stream) {
  const LpWfParams f{part, dw, nwg, ncp, ncqg, nslot, ntaps, NQ, Cp, Cq, Cin_ref, dup_start, dup_shift, accum};
  const bool four = ntaps == 27 && nslot == 27 && Cq % 4 == 0 && (((uintptr_t)part) & 15) == 0;
  const long total = (long)ntaps * Cp * Cq;
  long blocks = ((four ? total / 4 : total) + 31) / 32;
  if (blocks > 8192) blocks = 8192;
  (void)hipGetLastError();
  hipLaunchKernelGGL(four ? lp_wgrad_finalize4_kernel : lp_wgrad_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, f);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
// db[k] (+)= sum_n colsum[n][k]
__global__ void lp_bias_grad_kernel(const float* cs, float* db, int N, int C, int accum) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= C) return;
  float s = 0.f;
  for (int n = 0; n < N; ++n) s += cs[n * C + k];
  db[k] = accum ? db[k] + s : s;
}

// ---- plan: one choice per call (lowp_common.h) ----
bool lp_wg_accept(const LpWgCall& c, LpWgChoice& ch) {
  if (c.kind != BTS_CONV_K3S1 && c.kind != BTS_CONV_K1) return false;
  if (c.gna_G != 0 || c.k1f != 0 || c.x_split != 0) return false;
  LpWgPlan& g = ch.g;
  lp_wg_tiles(g, c.N, c.Cin, c.Cout, (c.W + LPW_TX - 1) / LPW_TX, (c.H + LPW_TY - 1) / LPW_TY, (c.D + LPW_TZ - 1) / LPW_TZ);
  ch.kernel = LP_WG;
  ch.part = (long)g.nwg * g.ncp * g.ncqg * (c.kind == BTS_CONV_K3S1 ? 27 : 8) * 32 * 32 * g.nq * 4;
  return true;
}
// what the entry points refuse whatever the kernel, in the order they have always reported it; the db rules are bts_lp_colsum's, asked
// BEFORE anything is launched: a call that cannot produce its db leaves dw alone
static int lp_wg_args(const LpWgCall& c, bool strided) {
  if (c.Cin % 8 != 0 || c.Cout % 8 != 0 || c.ldx % 8 != 0 || c.lddy % 8 != 0) return BTS_ERR_SHAPE;      // (16-byte chunks of channels)
  if (c.kind == BTS_CONV_K3S2 && ((c.D | c.H | c.W) & 1)) return BTS_ERR_UNSUPPORTED;
  if (strided && c.dup_shift != 0) return BTS_ERR_UNSUPPORTED;
  if (!c.aligned) return BTS_ERR_ALIGN;
  if (c.dup_shift < 0 || (c.dup_shift > 0 && c.dup_start + c.dup_shift > c.Cin)) return BTS_ERR_SHAPE;
  if (c.want_db && c.lddy != c.Cout) return BTS_ERR_UNSUPPORTED;
  if (c.want_db && (c.Cout > 256 || 256 % (c.Cout / 8) != 0)) return BTS_ERR_SHAPE;
  return BTS_OK;
}
int lp_wg_choose(const LpWgCall& c, LpWgChoice& ch) {
  ch = LpWgChoice{};
  const bool strided = c.kind == BTS_CONV_K3S2 || c.kind == BTS_CONV_K3S2T;
  if (!strided && c.kind != BTS_CONV_K3S1 && c.kind != BTS_CONV_K1) return BTS_ERR_UNSUPPORTED;
  if (c.N <= 0 || c.D <= 0 || c.H <= 0 || c.W <= 0 || c.Cin <= 0 || c.Cout <= 0) return BTS_ERR_SHAPE;
  const int st = lp_wg_args(c, strided);
  if (strided) {
    if (!lp_wgs_accept(c, ch)) return st != BTS_OK ? st : BTS_ERR_SHAPE;      // (its 31-bit offsets)
  } else {
    // the streaming kernel is offered first; the general one takes every call without a form.  Their slabs sit in the same place and the area
    // holds the larger: a launch whose strides turn the streaming kernel away still fits the workspace its dense query sized.
    LpWgChoice d{};
    lp_wg_accept(c, ch);
    if (lp_wgd_accept(c, d)) {
      if (d.part < ch.part) d.part = ch.part;
      ch = d;
    }
    if (ch.kernel == 0) return st != BTS_OK ? st : 1;
  }
  // workspace: [partial slabs | per-sample column sums of dy | bts_lp_colsum's workspace]  (the slack is what the queries have always answered)
  const int C8 = (c.Cout + 7) / 8 * 8;
  ch.cs_off = ch.part;
  ch.cws_off = ch.cs_off + (((long)c.N * C8 * 4 + 255) & ~255L);
  ch.ws = ch.part + (long)c.N * C8 * 4 + bts_lp_colsum_workspace(c.N, lp_wg_dy_voxels(c), C8) + (strided || c.k1f ? 512 : 256);
  return st;
}
// the call as a workspace query sees it: dense operands, one tensor
static LpWgCall lp_wg_dense(LpWgCall c) {
  c.ldx = c.Cin; c.lddy = c.Cout; c.lddy1 = c.k1f ? c.Cout : 0;
  c.x_split = 0; c.want_db = 0; c.aligned = 1;
  return c;
}
static bool lp_wg_aligned(const void* a, const void* b, const void* c, const void* d = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

// ---- launch ----
static int lp_wg_launch(int dtype, const LpWgCall& c, const LpWgChoice& ch, const LpWgPtrs& q, hipStream_t stream) {
  const LpWgPlan& g = ch.g;
  const bool k3 = c.kind == BTS_CONV_K3S1;
  const int nq = g.nq, nwg = g.nwg;
  LpWgParams p;
  p.p = (const unsigned short*)q.x; p.q = (const unsigned short*)q.dy; p.part = reinterpret_cast<float*>(q.ws);
  p.N = c.N; p.D = c.D; p.H = c.H; p.W = c.W; p.Cp = c.Cin; p.ldp = c.ldx; p.Cq = c.Cout; p.ldq = c.lddy; p.ntaps = k3 ? 27 : 1;
  p.ntx = g.ntx; p.nty = g.nty; p.ntz = g.ntz; p.ntiles = g.ntiles; p.ncp = g.ncp; p.ncqg = g.ncqg;
  const size_t shmem = ((size_t)(LPW_TX + 2) * (LPW_TY + 2) * (LPW_TZ + 2) * 36 + (size_t)LPW_TX * LPW_TY * LPW_TZ * (32 * nq + 4)) * 2;
  (void)hipGetLastError();
#define LPW_LAUNCH(TT, NQ_, K3_)                                                                                                \
  do {                                                                                                                        \
    auto kern = lp_wgrad_kernel<TT, NQ_, K3_>;                                                                                \
    static bool done = false;                                                                                                 \
    if (!done) {                                                                                                              \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
      if (e != hipSuccess) return (int)e;                                                                                     \
      done = true;                                                                                                            \
    }                                                                                                                         \
    hipLaunchKernelGGL(kern, dim3(nwg, p.ncp * p.ncqg), dim3(512), shmem, stream, p);                                         \
  } while (0)
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(32 | ((k3 ? 1 : 2) << 16), 2.0 * p.ntaps * (double)c.Cin * c.Cout * (double)c.N * c.D * c.H * c.W, stream);   // (variant 2: 1x1x1 -- 2 FLOP per operand byte, HBM-bound)
  // (the launch macro's `return` on a failed hipFuncSetAttribute leaves the lambda: its status is handed on here)
  const int lr = lp_typed(dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (k3) { if (nq == 2) LPW_LAUNCH(T, 2, true); else LPW_LAUNCH(T, 1, true); }
    else { if (nq == 2) LPW_LAUNCH(T, 2, false); else LPW_LAUNCH(T, 1, false); }
    return BTS_OK;
  });
  if (lr != BTS_OK) return lr;
#undef LPW_LAUNCH
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return bts_lp_wgrad_finalize_(p.part, q.dw, nwg, g.ncp, g.ncqg, k3 ? 27 : 8, p.ntaps, nq, c.Cin, c.Cout, c.Cin + c.dup_shift, c.dup_start,
                                c.dup_shift, c.accum, stream);
}
// db (+)= sum of dy over voxels and samples (dy dense: lp_wg_choose has checked); db NULL: nothing
static int lp_wg_bias_tail(int dtype, const LpWgCall& c, const LpWgChoice& ch, const void* dy, float* db, void* ws, hipStream_t stream) {
  if (db == nullptr) return BTS_OK;
  char* wsb = reinterpret_cast<char*>(ws);
  float* cs = reinterpret_cast<float*>(wsb + ch.cs_off);
  const long V = lp_wg_dy_voxels(c);
  const int r = bts_lp_colsum(dtype, dy, cs, wsb + ch.cws_off, bts_lp_colsum_workspace(c.N, V, c.Cout), c.N, V, c.Cout, 1.0f, stream);
  if (r != BTS_OK) return r;
  hipLaunchKernelGGL(lp_bias_grad_kernel, dim3((c.Cout + 255) / 256), dim3(256), 0, stream, cs, db, c.N, c.Cout, c.accum);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
// the chosen kernel (+ finalize), then the bias gradient
static int lp_wg_run(int dtype, const LpWgCall& c, const LpWgChoice& ch, const LpWgPtrs& q, float* db, hipStream_t stream) {
  const int r = ch.kernel == LP_WGD ? bts_lp_wgd_launch_(dtype, c, ch, q, stream)
              : ch.kernel == LP_WGS ? bts_lp_wgs_launch_(dtype, c, ch, q, stream) : lp_wg_launch(dtype, c, ch, q, stream);
  return r != BTS_OK ? r : lp_wg_bias_tail(dtype, c, ch, q.dy, db, q.ws, stream);
}

// ---- queries and entry points (conventions: bts_hip.h).  Launch-side rule: the workspace was sized by a query that saw dense operands; the
// launch chooses again for the strides it is given and needs both what that query answered and what its own choice takes ----
extern "C" long bts_lp_conv3d_bwd_weight_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  LpWgCall c{kind, N, D, H, W, Cin, Cin, Cout, Cout};
  LpWgChoice ch;
  lp_wg_choose(lp_wg_dense(c), ch);      // (a size for every channel count: what a launch refuses is the launch's to say)
  return ch.kernel != 0 ? ch.ws : -1;
}
// x on the forward-input grid; dy on the same grid (K3S1, K1), the half grid (K3S2: TF 'same' with even sizes pads (0,1): input 2o + t) or the
// doubled grid (K3S2T: output 2i + k)
extern "C" int bts_lp_conv3d_bwd_weight(int kind, int dtype, const void* x, const void* dy, float* dw, float* db, void* workspace,
                                        long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int dup_start,
                                        int dup_shift, int accumulate, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  LpWgCall c{kind, N, D, H, W, Cin, ldx, Cout, lddy, dup_start, dup_shift, accumulate, db != nullptr};
  c.aligned = lp_wg_aligned(x, dy, workspace);
  LpWgChoice ch, sized;
  const int r = lp_wg_choose(c, ch);
  if (r != BTS_OK) return r;
  if (lp_wg_choose(lp_wg_dense(c), sized) != BTS_OK || workspace_bytes < sized.ws || workspace_bytes < ch.ws) return BTS_ERR_WORKSPACE;
  return lp_wg_run(dtype, c, ch, LpWgPtrs{x, dy, dw, workspace}, db, stream);
}
// lp_wg_args' answer for the dense, aligned, unfolded call (conventions: bts_hip.h); the stride-1 kinds are asked with a bias gradient
extern "C" int bts_lp_conv3d_bwd_weight_args_ok(int kind, int D, int H, int W, int Cin, int Cout) {
  const bool strided = kind == BTS_CONV_K3S2 || kind == BTS_CONV_K3S2T;
  if (!strided && kind != BTS_CONV_K3S1 && kind != BTS_CONV_K1) return 0;
  if (D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  LpWgCall c{kind, 1, D, H, W, Cin, Cin, Cout, Cout};
  c.want_db = strided ? 0 : 1;
  c.aligned = 1;
  return lp_wg_args(c, strided) == BTS_OK ? 1 : 0;
}
// conv1's and the shortcut's weight gradients from ONE pass over the block input (K1F: the 1x1x1 gradient is one more accumulator per wave of
// the streaming kernel; conventions: bts_hip.h).  Query -1 / call 1 (nothing launched) where that kernel does not take the shape.
static LpWgCall lp_wg_pair_call(int N, int D, int H, int W, int Cin, int Cout) {
  LpWgCall c{BTS_CONV_K3S1, N, D, H, W, Cin, Cin, Cout, Cout};
  c.k1f = 1;
  return lp_wg_dense(c);
}
extern "C" long bts_lp_conv3d_bwd_weight_pair_workspace(int N, int D, int H, int W, int Cin, int Cout) {
  LpWgChoice ch;
  return lp_wg_choose(lp_wg_pair_call(N, D, H, W, Cin, Cout), ch) == BTS_OK ? ch.ws : -1;
}
extern "C" int bts_lp_conv3d_bwd_weight_pair(int dtype, const void* x, long x_split, const void* dy3, const void* dy1, float* dw3, float* dw1,
                                             float* db3, void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx,
                                             int Cout, int lddy3, int lddy1, int dup_start, int dup_shift, int accumulate, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  LpWgChoice ch, sized;
  if (lp_wg_choose(lp_wg_pair_call(N, D, H, W, Cin, Cout), sized) != BTS_OK) return 1;      // (where the query says -1)
  if (x == nullptr || dy3 == nullptr || dy1 == nullptr || dw3 == nullptr || dw1 == nullptr) return BTS_ERR_ALIGN;
  if (ldx % 8 != 0 || lddy3 % 8 != 0 || lddy1 % 8 != 0 || ldx < (x_split ? 32 : Cin) || lddy3 < Cout || lddy1 < Cout) return BTS_ERR_SHAPE;
  if (x_split != 0 && (x_split < 0 || x_split % 8 != 0 || Cin % 32 != 0 || dup_shift != 0)) return BTS_ERR_SHAPE;
  LpWgCall c{BTS_CONV_K3S1, N, D, H, W, Cin, ldx, Cout, lddy3, dup_start, dup_shift, accumulate, db3 != nullptr};
  c.k1f = 1; c.lddy1 = lddy1; c.x_split = x_split;
  c.aligned = lp_wg_aligned(x, dy3, dy1, workspace);
  if (workspace == nullptr || workspace_bytes < sized.ws) return BTS_ERR_WORKSPACE;
  const int r = lp_wg_choose(c, ch);      // (1: these strides leave the streaming kernel's 31-bit offsets -- nothing launched)
  if (r != BTS_OK) return r;
  return lp_wg_run(dtype, c, ch, LpWgPtrs{x, dy3, dw3, workspace, nullptr, dy1, dw1}, db3, stream);
}
// conv2 of a ResnetBlock in TRAINING without the normalised tensor (GNA: the streaming kernel normalises its P planes, the raw x, in LDS;
// conventions: bts_hip.h).  bts_lp_conv3d_gnin_train_ok: 1 when BOTH kernels take the shape in this form (ask before the forward), else 0.
extern "C" int bts_lp_conv3d_gnin_train_ok(int N, int D, int H, int W, int Cin, int Cout, int in_G, int G) {
  if (bts_lp_conv3d_gnin_fwd_gn_workspace(N, D, H, W, Cin, Cout, in_G, G) < 0) return 0;
  LpWgCall c{BTS_CONV_K3S1, N, D, H, W, Cin, Cin, Cout, Cout};
  c.gna_G = in_G;
  LpWgChoice ch;
  return in_G > 0 && lp_wg_choose(lp_wg_dense(c), ch) == BTS_OK ? 1 : 0;
}
// workspace: bts_lp_conv3d_bwd_weight_workspace(BTS_CONV_K3S1, ...).  BTS_ERR_UNSUPPORTED where bts_lp_conv3d_gnin_train_ok says 0.
extern "C" int bts_lp_conv3d_gnin_bwd_weight(int dtype, const void* x, const float* in_gamma, const float* in_beta, const float* in_mean,
                                             const float* in_rstd, int in_G, const void* dy, float* dw, float* db, void* workspace,
                                             long workspace_bytes, int N, int D, int H, int W, int Cin, int Cout, int lddy, int accumulate,
                                             hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (lddy < Cout) return BTS_ERR_SHAPE;
  LpWgCall c{BTS_CONV_K3S1, N, D, H, W, Cin, Cin, Cout, lddy, 0, 0, accumulate, db != nullptr};
  c.gna_G = in_G;
  c.aligned = lp_wg_aligned(x, dy, workspace);
  LpWgChoice ch;
  const int r = lp_wg_choose(c, ch);      // (rows of lddy >= Cout reach at least as far as dense ones: what train_ok refuses, this refuses)
  if (r != BTS_OK && r != 1) return r;
  if (r == 1 || in_G <= 0) return BTS_ERR_UNSUPPORTED;
  if (workspace_bytes < bts_lp_conv3d_bwd_weight_workspace(BTS_CONV_K3S1, N, D, H, W, Cin, Cout)) return BTS_ERR_WORKSPACE;
  const LpGnaFuse ga{in_gamma, in_beta, in_mean, in_rstd, in_G, Cin / in_G};
  return lp_wg_run(dtype, c, ch, LpWgPtrs{x, dy, dw, workspace, &ga}, db, stream);
}
