// Weight (and bias) gradients of the 3-D convolutions on the exact-fp32 matrix pipe.
// The reference obtains these from TF autodiff (train.py:142-151); the math is SURVEY Appendix A':
//   dW[t][pc][qc] = sum_{n,v} P[n, v*s + off_t, pc] * Q[n, v, qc]        db[qc] = sum_{n,v} Q[n, v, qc]
//     Conv3D k1 / k3s1 / k3s2 : P = layer input x, Q = dy  -> dW in (t, Cin, Cout)
//     Conv3DTranspose k3s2    : P = dy (fine grid, s=2), Q = x (coarse grid) -> dW in (t, Cout, Cin)
//     "swapped" k3s1          : P = dy, Q = x with negated tap offsets (u = v + off_t): used when Cout <= 8 so the
//                               tiny channel count sits on the packable P side
// GEMM view: M = 32 rows (P channels of one tap, or -- when P has <= 16 channels -- packed (tap, channel) pairs),
// N = 32 Q-channels, K = voxels (v_mfma_f32_32x32x2_f32 consumes 2 voxels per instruction).
// A 512-thread workgroup (8 waves) walks a run of spatial sub-tiles; the waves split the row-tiles (27 taps) or, when
// there are at most 4 row-tiles, the voxel pairs.  P halo tile and Q tile live in LDS as [voxel][channels] so both
// fragment reads are conflict-free ds_read_b32; the next sub-tile is staged by direct global->LDS DMA
// (global_load_lds_dwordx4) while the current one is multiplied (double-buffered LDS, one barrier per sub-tile).
// Kernel variants <MODE, FIXG>: <2,1>/<2,2> straight-line fixed-geometry sweeps with interleaved staging for every big
// 3x3x3 layer (stride 1 / 2), <1,0> general LDS-DMA staging, <0,0> register staging for odd strides / channel counts.
// Per-workgroup partials go to a workspace and are combined in a fixed order by the finalize kernel (bitwise
// reproducible; no float atomics).
#include <stdlib.h>
#include <type_traits>
#include "common.h"
#include "bts_internal.h"

#define WG_THREADS 512
#define WG_WAVES 8
#define WG_MAXT 4
#define WG_PSLOTS 8
#define WG_QSLOTS 4

struct WgradParams {
  const float* p;
  const float* q;
  float* partial;     // [nsp][npct][nqct][ntiles][32][32]
  double* partial_b;  // [nsp][nqct][32]
  const float* zeros;  // >= 16 zero bytes (source for padding lanes of the LDS-DMA staging)
  int N, Dp, Hp, Wp, Cp, ldp;
  int Dq, Hq, Wq, Cq, ldq;
  int s, loz, loy, lox;
  int IZ, IY, IX;
  int lgTX, lgTY, TZ;
  int ntz, nty, ntx;
  int ntaps, ntiles, cpad, lgSP;
  int nsub, sub_per_wg;
  int want_bias;
  int fixg;  // 1/2: the sub-tile is the unclamped 16x4x2 (stride 1) / 8x4x1 (stride 2) 27-tap geometry -> fixed sweep
  int fastf;  // fixed geometry AND whole tiles / whole 32-channel groups: per-lane staging offsets are precomputed once
  int tap_vox[27];  // voxel offset of each tap inside the P halo tile
};

__device__ __forceinline__ int fast_div(int a, float inv) { return (int)(((float)a + 0.5f) * inv); }

// MFMA sweep over the voxel pairs ("steps") of one staged sub-tile for a wave that owns T row-tiles.
// Software pipelined by hand: the LDS reads of step k+1 are issued before the T MFMAs of step k, so LDS latency and the
// address arithmetic sit in the shadow of the matrix pipe.  Step indices are wave-uniform (scalar address part); the
// per-lane part (row offset of the tile, half-wave voxel, channel) is folded into laneoff[] once.
// The fragment reads are inline-asm ds_read_b32 with hand-counted s_waitcnt lgkmcnt(N): hipcc cannot count LDS
// operations across the loop back-edge and would otherwise wait lgkmcnt(0) right after issuing the prefetch.
template <int T>
struct WgFrag {
  float q, a[T];
};
__device__ __forceinline__ float lds_read_b32_async(unsigned byte_addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(byte_addr));
  return v;
}
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int T>
__device__ __forceinline__ void wgrad_steps(const WgradParams& p, const float* bp, const float* bq, const int (&rowoff)[WG_MAXT],
                                            f32x16 (&acc)[WG_MAXT], int st0, int stinc, int nsteps, int h, int l32) {
  const int TXm = (1 << p.lgTX) - 1, TYm = (1 << p.lgTY) - 1, lgXY = p.lgTX + p.lgTY;
  const unsigned bpb = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)bp;  // LDS byte addresses
  const unsigned bqb = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)bq;
  unsigned laneoff[T];
#pragma unroll
  for (int i = 0; i < T; ++i) laneoff[i] = bpb + 4u * (unsigned)(rowoff[i] + ((h * p.s) << p.lgSP));
  const unsigned qlane = bqb + 4u * (unsigned)(h * 32 + l32);
  const int nK = (nsteps - st0 + stinc - 1) / stinc;
  auto load = [&](WgFrag<T>& f, int k) {
    const int m = 2 * (st0 + k * stinc);  // wave-uniform
    const int pvu = (((m >> lgXY) * p.s * p.IY + ((m >> p.lgTX) & TYm) * p.s) * p.IX + (m & TXm) * p.s) << p.lgSP;
    f.q = lds_read_b32_async(qlane + (unsigned)(m * 128));
#pragma unroll
    for (int i = 0; i < T; ++i) f.a[i] = lds_read_b32_async(laneoff[i] + (unsigned)(pvu * 4));
    __builtin_amdgcn_sched_barrier(0);
  };
  // One step = T MFMAs on the fragment fetched one step earlier.  The next fragment's address arithmetic and LDS reads
  // are issued right after the first MFMA so they retire in the shadow of the matrix pipe (a wave blocks on MFMA issue
  // while the pipe is busy; anything placed before the burst would instead serialise with it), and the burst runs at
  // raised priority so the two waves of a SIMD alternate whole bursts instead of dragging each other through them
  // (scripts/ubench/mfma_lds_feed.hip: 142 -> 154 TFLOP/s at 2 waves/SIMD).
  auto step = [&](const WgFrag<T>& cur, WgFrag<T>& nxt, int knext) {
    wait_lgkm<0>();
    __builtin_amdgcn_s_setprio(1);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[0], cur.q, acc[0], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    load(nxt, knext);
#pragma unroll
    for (int i = 1; i < T; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[i], cur.q, acc[i], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  WgFrag<T> A, B;
  if (nK <= 0) return;
  load(A, 0);
  const int last = nK - 1;
  for (int k = 0; k < nK; k += 2) {
    step(A, B, k + 1 < last ? k + 1 : last);  // the final prefetch re-reads the last fragment (never consumed)
    if (k + 1 >= nK) break;
    step(B, A, k + 2 < last ? k + 2 : last);
  }
  wait_lgkm<0>();
}

// ---- fixed-geometry sweep (3x3x3 taps, 32-channel P voxels, unclamped sub-tile) ---------------------------------------
// Measured cost model (scripts/ubench/wgrad_sweep.hip): next to the matrix pipe EVERY issued instruction costs ~4 cycles
// of SIMD time, scalar ones included, so the general step above (13 SALU + 6 VALU + T+1 LDS reads per T MFMAs) tops out
// at ~105 TFLOP/s.  Here the sub-tile geometry is a template parameter and the whole sub-tile is one straight-line
// sequence: every voxel offset is a DS immediate off T+1 per-wave base registers (tile base + tap offset of row-tile i),
// a step is T+1 ds_read_b32 + T MFMAs and nothing else.  The staging of the NEXT sub-tile is not issued up front by all
// waves at once but handed in as `stage(IC<K>)`, a few instructions at a time in the MFMA shadow of chosen steps.
template <int I>
struct IC { static constexpr int value = I; };
template <int S, int TX, int TY, int TZ>
struct WgGeo {
  static constexpr int IX = (TX - 1) * S + 3, IY = (TY - 1) * S + 3;
  static constexpr int JR = TX / 2;       // voxel-pair steps per x-row
  static constexpr int NS = JR * TY * TZ;  // steps per sub-tile
  // P byte offset (before the tap offset) of the first voxel of step K; Q is simply [m][32]
  static constexpr int p_b(int K) {
    const int r = K / JR, j = K % JR, z = r / TY, y = r % TY;
    return ((z * S * IY + y * S) * IX + 2 * j * S) * 128;
  }
};
template <int T, typename G, int K>
__device__ __forceinline__ void wgx_load(WgFrag<T>& f, const unsigned (&vp)[WG_MAXT], unsigned vq) {
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f.q) : "v"(vq), "n"(K * 256));
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f.a[0]) : "v"(vp[0]), "n"(G::p_b(K)));
  if constexpr (T > 1) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f.a[1]) : "v"(vp[1]), "n"(G::p_b(K)));
  if constexpr (T > 2) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f.a[2]) : "v"(vp[2]), "n"(G::p_b(K)));
  if constexpr (T > 3) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f.a[3]) : "v"(vp[3]), "n"(G::p_b(K)));
  __builtin_amdgcn_sched_barrier(0);
}
// Three rotating fragments: the reads of step K+2 are issued in step K, so a fragment has two full MFMA bursts to land.
// lgkmcnt(T+1): LDS operations retire in order, so at most the T+1 youngest (fragment K+1) are still in flight.
template <int T, typename G, int K, typename F>
__device__ __forceinline__ void wgx_steps(WgFrag<T>& f0, WgFrag<T>& f1, WgFrag<T>& f2, f32x16 (&acc)[WG_MAXT],
                                          const unsigned (&vp)[WG_MAXT], unsigned vq, F& stage) {
  if constexpr (K + 1 < G::NS) wait_lgkm<T + 1>();
  else wait_lgkm<0>();
  __builtin_amdgcn_s_setprio(1);
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f0.a[0], f0.q, acc[0], 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K + 2 < G::NS) wgx_load<T, G, K + 2>(f2, vp, vq);
  stage(IC<K>{});
  if constexpr (K + 2 >= G::NS && K + 1 < G::NS) wait_lgkm<T + 1>();  // staging writes issued here must not hide fragment K+1
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 1; i < T; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(f0.a[i], f0.q, acc[i], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K + 1 < G::NS) wgx_steps<T, G, K + 1>(f1, f2, f0, acc, vp, vq, stage);
}
template <int T, typename G, typename F>
__device__ __forceinline__ void wgrad_sweep_fixed(const unsigned (&vp)[WG_MAXT], unsigned vq, f32x16 (&acc)[WG_MAXT], F& stage) {
  WgFrag<T> A, B, C;
  wgx_load<T, G, 0>(A, vp, vq);
  wgx_load<T, G, 1>(B, vp, vq);
  wgx_steps<T, G, 0>(A, B, C, acc, vp, vq, stage);
  wait_lgkm<0>();
}

// GLDS = true: tiles are staged with direct global->LDS DMA (global_load_lds_dwordx4: no staging registers, the copy of
// the next sub-tile is fully asynchronous under the MFMA sweep).  The LDS image is lane-linear by construction (slot e
// lives at byte 16*e), padding lanes read 16 zero bytes from p.zeros.  GLDS = false: register-staged fallback for
// channel counts / strides that are not 16-byte granular.
// MODE 0: register staging, 1: LDS-DMA staging, 2: LDS-DMA staging with precomputed slot offsets (p.fastf).
// FIXG 0: general sweep, 1/2: fixed-geometry sweep (p.fixg).  Separate kernels so each keeps its own register budget.
template <int MODE, int FIXG>
__global__ __launch_bounds__(WG_THREADS, 2) void wgrad_kernel(const WgradParams p) {
  constexpr bool GLDS = MODE >= 1, FAST = MODE == 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  const int pct = blockIdx.y, qct = blockIdx.z;
  const int TX = 1 << p.lgTX, TY = 1 << p.lgTY;
  const int M = TX * TY * p.TZ;
  const int SP = 1 << p.lgSP;
  const int tileVoxP = p.IZ * p.IY * p.IX;
  const int pRegion = ((tileVoxP * (SP >> 2) + 63) & ~63) * 4;  // dwords, padded to whole wave-loads (64 x 16 B)
  const int qRegion = ((M * 8 + 63) & ~63) * 4;
  const int bufDw = pRegion + qRegion;
  const bool ksplit = p.ntiles <= WG_MAXT;  // few row-tiles: every wave takes all of them, waves split the voxel pairs

  // ---- per-lane row offsets (dwords inside the P tile) for this wave's row-tiles ----
  int rowoff[WG_MAXT];
#pragma unroll
  for (int i = 0; i < WG_MAXT; ++i) {
    const int tile = ksplit ? i : wave + WG_WAVES * i;
    int off = 0;
    if (tile < p.ntiles) {
      if (p.cpad == 32) off = (p.tap_vox[tile] << p.lgSP) + l32;
      else {
        const int ci = tile * 32 + l32;
        int tap = ci / p.cpad;
        const int ch = ci - tap * p.cpad;
        if (tap >= p.ntaps) tap = 0;  // junk row, never read back
        off = (p.tap_vox[tap] << p.lgSP) + ch;
      }
    }
    rowoff[i] = off;
  }

  int ntw = 0;  // row-tiles owned by this wave
#pragma unroll
  for (int i = 0; i < WG_MAXT; ++i) {
    const int tile = ksplit ? i : wave + WG_WAVES * i;
    if (tile < p.ntiles) ntw = i + 1;
  }

  const int qpvP = SP >> 2;  // float4 per P voxel
  const float invIX = 1.0f / (float)p.IX, invIYX = 1.0f / (float)(p.IY * p.IX);
  // Staging slots: slot e of a tile covers float4 #e of its LDS image ([voxel][SP] resp. [m][32]), so the LDS offset is
  // simply 4*e; the voxel decomposition is recomputed per sub-tile (a dozen VALU ops) rather than kept in registers:
  // spilled slot tables would be reloaded through the VM counter and serialise the prefetch loads.
  const int pc0 = pct * 32;
  const int nPslots = tileVoxP * qpvP, nQslots = M * 8;
  const int IYX = p.IY * p.IX;
  const int vecP = (p.ldp % 4 == 0) && (p.Cp % 4 == 0) && ((((uintptr_t)p.p) & 15) == 0);
  const int vecQ = (p.ldq % 4 == 0) && (p.Cq % 4 == 0) && ((((uintptr_t)p.q) & 15) == 0);

  f32x4 preP[WG_PSLOTS], preQ[WG_QSLOTS];
  auto fetch = [&](int sub) {
    int b = sub;
    const int tx = b % p.ntx; b /= p.ntx;
    const int ty = b % p.nty; b /= p.nty;
    const int tz = b % p.ntz;
    const int n = b / p.ntz;
    const int oz0 = tz * p.TZ, oy0 = ty * TY, ox0 = tx * TX;
    const int iz0 = oz0 * p.s + p.loz, iy0 = oy0 * p.s + p.loy, ix0 = ox0 * p.s + p.lox;
    // wave-uniform tile origins (may be negative for the halo): pointer arithmetic stays scalar
    const float* pbase = p.p + ((((long)n * p.Dp + iz0) * p.Hp + iy0) * p.Wp + ix0) * (long)p.ldp;
    const float* qbase = p.q + ((((long)n * p.Dq + oz0) * p.Hq + oy0) * p.Wq + ox0) * (long)p.ldq;
#pragma unroll
    for (int i = 0; i < WG_PSLOTS; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      const int e = tid + i * WG_THREADS;
      if (e < nPslots) {
        const int vox = e >> (p.lgSP - 2), qd = e & (qpvP - 1);
        const int vz = fast_div(vox, invIYX);
        const int r = vox - vz * IYX;
        const int vy = fast_div(r, invIX);
        const int vx = r - vy * p.IX;
        const int c = pc0 + qd * 4;
        if ((unsigned)(iz0 + vz) < (unsigned)p.Dp && (unsigned)(iy0 + vy) < (unsigned)p.Hp &&
            (unsigned)(ix0 + vx) < (unsigned)p.Wp && c < p.Cp) {
          const float* src = pbase + (((vz * p.Hp + vy) * p.Wp + vx) * p.ldp + c);
          if (vecP) v = *reinterpret_cast<const f32x4*>(src);
          else {
            v[0] = src[0];
            if (c + 1 < p.Cp) v[1] = src[1];
            if (c + 2 < p.Cp) v[2] = src[2];
            if (c + 3 < p.Cp) v[3] = src[3];
          }
        }
      }
      preP[i] = v;
    }
#pragma unroll
    for (int i = 0; i < WG_QSLOTS; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      const int e = tid + i * WG_THREADS;
      if (e < nQslots) {
        const int m = e >> 3, qd = e & 7;
        const int mz = m >> (p.lgTX + p.lgTY), my = (m >> p.lgTX) & (TY - 1), mx = m & (TX - 1);
        const int c = qct * 32 + qd * 4;
        if (oz0 + mz < p.Dq && oy0 + my < p.Hq && ox0 + mx < p.Wq && c < p.Cq) {
          const float* src = qbase + (((mz * p.Hq + my) * p.Wq + mx) * p.ldq + c);
          if (vecQ) v = *reinterpret_cast<const f32x4*>(src);
          else {
            v[0] = src[0];
            if (c + 1 < p.Cq) v[1] = src[1];
            if (c + 2 < p.Cq) v[2] = src[2];
            if (c + 3 < p.Cq) v[3] = src[3];
          }
        }
      }
      preQ[i] = v;
    }
  };
  // direct-to-LDS staging of one sub-tile into buffer `buf` (every lane of every issuing wave is active)
  auto fetch_glds = [&](int sub, float* buf) {
    int b = sub;
    const int tx = b % p.ntx; b /= p.ntx;
    const int ty = b % p.nty; b /= p.nty;
    const int tz = b % p.ntz;
    const int n = b / p.ntz;
    const int oz0 = tz * p.TZ, oy0 = ty * TY, ox0 = tx * TX;
    const int iz0 = oz0 * p.s + p.loz, iy0 = oy0 * p.s + p.loy, ix0 = ox0 * p.s + p.lox;
    const float* pbase = p.p + ((((long)n * p.Dp + iz0) * p.Hp + iy0) * p.Wp + ix0) * (long)p.ldp;
    const float* qbase = p.q + ((((long)n * p.Dq + oz0) * p.Hq + oy0) * p.Wq + ox0) * (long)p.ldq;
#pragma unroll
    for (int i = 0; i < WG_PSLOTS; ++i) {
      const int e0 = wave * 64 + i * WG_THREADS;  // wave-uniform first slot of this wave-load
      if (e0 * 4 < pRegion) {
        const int e = e0 + lane;
        const float* src = p.zeros;
        if (e < nPslots) {
          const int vox = e >> (p.lgSP - 2), qd = e & (qpvP - 1);
          const int vz = fast_div(vox, invIYX);
          const int r = vox - vz * IYX;
          const int vy = fast_div(r, invIX);
          const int vx = r - vy * p.IX;
          const int c = pc0 + qd * 4;
          if ((unsigned)(iz0 + vz) < (unsigned)p.Dp && (unsigned)(iy0 + vy) < (unsigned)p.Hp &&
              (unsigned)(ix0 + vx) < (unsigned)p.Wp && c < p.Cp)
            src = pbase + (((vz * p.Hp + vy) * p.Wp + vx) * p.ldp + c);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(buf + e0 * 4), 16, 0, 0);
      }
    }
    float* bqd = buf + pRegion;
#pragma unroll
    for (int i = 0; i < WG_QSLOTS; ++i) {
      const int e0 = wave * 64 + i * WG_THREADS;
      if (e0 * 4 < qRegion) {
        const int e = e0 + lane;
        const float* src = p.zeros;
        if (e < nQslots) {
          const int m = e >> 3, qd = e & 7;
          const int mz = m >> (p.lgTX + p.lgTY), my = (m >> p.lgTX) & (TY - 1), mx = m & (TX - 1);
          const int c = qct * 32 + qd * 4;
          if (oz0 + mz < p.Dq && oy0 + my < p.Hq && ox0 + mx < p.Wq && c < p.Cq)
            src = qbase + (((mz * p.Hq + my) * p.Wq + mx) * p.ldq + c);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(bqd + e0 * 4), 16, 0, 0);
      }
    }
  };
  // Fast staging (p.fastf): slot -> (voxel, channel quad) never changes, so the byte offset of every slot relative to
  // the tile origin and its halo-face membership are computed ONCE; per sub-tile an interior tile costs one
  // global_load_lds (scalar base + 32-bit lane offset) per slot and nothing else -- next to the matrix pipe every
  // issued instruction costs ~4 cycles of SIMD time.  Face slots of boundary tiles are zero-filled with ds_write.
  unsigned relP[WG_PSLOTS], relQ[WG_QSLOTS], faceP[2] = {0u, 0u};
  if constexpr (FAST) {
#pragma unroll
    for (int i = 0; i < WG_PSLOTS; ++i) {
      const int e = wave * 64 + lane + i * WG_THREADS;
      int vz = -p.loz, vy = -p.loy, vx = -p.lox, qd = 0;  // padding lanes re-read an always-valid voxel (never consumed)
      unsigned face = 0;
      if (e < nPslots) {
        const int vox = e >> 3;
        qd = e & 7;
        vz = fast_div(vox, invIYX);
        const int r = vox - vz * IYX;
        vy = fast_div(r, invIX);
        vx = r - vy * p.IX;
        face = (vz == 0 ? 1u : 0u) | (vz == p.IZ - 1 ? 2u : 0u) | (vy == 0 ? 4u : 0u) | (vy == p.IY - 1 ? 8u : 0u) |
               (vx == 0 ? 16u : 0u) | (vx == p.IX - 1 ? 32u : 0u);
      }
      relP[i] = (unsigned)((((vz * p.Hp + vy) * p.Wp + vx) * p.ldp + pc0 + qd * 4) * 4);
      faceP[i >> 2] |= face << (8 * (i & 3));
    }
#pragma unroll
    for (int i = 0; i < WG_QSLOTS; ++i) {
      const int e = wave * 64 + lane + i * WG_THREADS;
      int mz = 0, my = 0, mx = 0, qd = 0;
      if (e < nQslots) {
        const int m = e >> 3;
        qd = e & 7;
        mz = m >> (p.lgTX + p.lgTY); my = (m >> p.lgTX) & (TY - 1); mx = m & (TX - 1);
      }
      relQ[i] = (unsigned)((((mz * p.Hq + my) * p.Wq + mx) * p.ldq + qct * 32 + qd * 4) * 4);
    }
  }
  // per-sub-tile staging state (wave-uniform), set by fast_prep and consumed by the per-slot issue functions
  const char* f_pbase = nullptr;
  const char* f_qbase = nullptr;
  unsigned f_tmask = 0;
  float* f_buf = nullptr;
  auto fast_prep = [&](int sub, float* buf) {
    int b = sub;
    const int tx = b % p.ntx; b /= p.ntx;
    const int ty = b % p.nty; b /= p.nty;
    const int tz = b % p.ntz;
    const int n = b / p.ntz;
    const int oz0 = tz * p.TZ, oy0 = ty * TY, ox0 = tx * TX;
    const int iz0 = oz0 * p.s + p.loz, iy0 = oy0 * p.s + p.loy, ix0 = ox0 * p.s + p.lox;
    f_pbase = reinterpret_cast<const char*>(p.p + ((((long)n * p.Dp + iz0) * p.Hp + iy0) * p.Wp + ix0) * (long)p.ldp);
    f_qbase = reinterpret_cast<const char*>(p.q + ((((long)n * p.Dq + oz0) * p.Hq + oy0) * p.Wq + ox0) * (long)p.ldq);
    // faces of the halo tile that lie outside the image (stride 1: one-voxel halo on both sides; stride 2: high side only)
    const unsigned lowf = p.loz < 0 ? 1u : 0u;
    f_tmask = ((tz == 0) ? lowf : 0u) | ((tz == p.ntz - 1) ? 2u : 0u) | ((ty == 0) ? 4u * lowf : 0u) |
              ((ty == p.nty - 1) ? 8u : 0u) | ((tx == 0) ? 16u * lowf : 0u) | ((tx == p.ntx - 1) ? 32u : 0u);
    f_buf = buf;
  };
  auto fast_slot_p = [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int e0 = wave * 64 + i * WG_THREADS;
    if (e0 * 4 < pRegion) {
      if (f_tmask == 0 || ((faceP[i >> 2] >> (8 * (i & 3))) & f_tmask) == 0)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(f_pbase + relP[i]),
                                         (__attribute__((address_space(3))) void*)(f_buf + e0 * 4), 16, 0, 0);
      else {
        int ln = lane;
        asm volatile("" : "+v"(ln));  // keep the 8 per-slot zero-fill addresses out of the sub-tile loop's live registers
        *reinterpret_cast<f32x4*>(f_buf + (e0 + ln) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  auto fast_slot_q = [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const int e0 = wave * 64 + i * WG_THREADS;
    if (e0 * 4 < qRegion)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(f_qbase + relQ[i]),
                                       (__attribute__((address_space(3))) void*)(f_buf + pRegion + e0 * 4), 16, 0, 0);
  };
  auto fetch_fast = [&](int sub, float* buf) {  // everything at once (prologue only)
    fast_prep(sub, buf);
    fast_slot_p(IC<0>{}); fast_slot_p(IC<1>{}); fast_slot_p(IC<2>{}); fast_slot_p(IC<3>{});
    fast_slot_p(IC<4>{}); fast_slot_p(IC<5>{}); fast_slot_p(IC<6>{}); fast_slot_p(IC<7>{});
    fast_slot_q(IC<0>{}); fast_slot_q(IC<1>{}); fast_slot_q(IC<2>{}); fast_slot_q(IC<3>{});
  };
  auto commit = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < WG_PSLOTS; ++i) {
      const int e = tid + i * WG_THREADS;
      if (e < nPslots) *reinterpret_cast<f32x4*>(buf + e * 4) = preP[i];
    }
    float* bq = buf + pRegion;
#pragma unroll
    for (int i = 0; i < WG_QSLOTS; ++i) {
      const int e = tid + i * WG_THREADS;
      if (e < nQslots) *reinterpret_cast<f32x4*>(bq + e * 4) = preQ[i];
    }
  };

  f32x16 acc[WG_MAXT];
#pragma unroll
  for (int i = 0; i < WG_MAXT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  // fixed-geometry kernels: partial accumulators of the three left-over row-tiles 24..26 (this wave's slice of K)
  f32x16 accx[WG_MAXT];
  int rowoffx[3] = {0, 0, 0};
  if constexpr (FIXG != 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) accx[i][r] = 0.f;
      rowoffx[i] = (p.tap_vox[24 + i] << p.lgSP) + l32;
    }
  }
  double bsum = 0.0;  // bias column sum: thread (c = tid&31, part = tid>>5)

  const int sub0 = blockIdx.x * p.sub_per_wg;
  int sub1 = sub0 + p.sub_per_wg;
  if (sub1 > p.nsub) sub1 = p.nsub;
  const int nsteps = M >> 1;

  if (sub0 < sub1) {
    if constexpr (GLDS) {
      if constexpr (FAST) fetch_fast(sub0, lds);
      else fetch_glds(sub0, lds);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      fetch(sub0);
      commit(lds);
    }
  }
  __syncthreads();
  int cur = 0;
  for (int sub = sub0; sub < sub1; ++sub) {
    const float* bp = lds + cur * bufDw;
    const float* bq = bp + pRegion;
    const bool more = (sub + 1) < sub1;
    if constexpr (FIXG == 0) {
      if (more) {
        if constexpr (GLDS) fetch_glds(sub + 1, lds + (cur ^ 1) * bufDw);
        else fetch(sub + 1);
      }
    }

    if (p.want_bias && pct == 0) {
      const int c = tid & 31, part = tid >> 5;
      float s = 0.f;
      for (int m = part; m < M; m += 16) s += bq[m * 32 + c];
      bsum += (double)s;
    }
    if constexpr (FIXG != 0) {
      using G = typename std::conditional<FIXG == 1, WgGeo<1, 16, 4, 2>, WgGeo<2, 8, 4, 1>>::type;
      // staging schedule: tile decode at step 0, then one slot every few steps (8 P + 4 Q slots per wave at most)
      constexpr int P0 = 1, PD = (G::NS >= 64) ? 5 : 1, Q0 = P0 + 8 * PD, QD = (G::NS >= 64) ? 5 : 1;
      static_assert(Q0 + 3 * QD < G::NS, "staging schedule does not fit the sub-tile");
      auto stage = [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if constexpr (K == 0) {
          if (more) fast_prep(sub + 1, lds + (cur ^ 1) * bufDw);
        } else if constexpr (K >= P0 && K < Q0 && (K - P0) % PD == 0) {
          if (more) fast_slot_p(IC<(K - P0) / PD>{});
        } else if constexpr (K >= Q0 && K <= Q0 + 3 * QD && (K - Q0) % QD == 0) {
          if (more) fast_slot_q(IC<(K - Q0) / QD>{});
        }
      };
      const unsigned bpb = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)bp;
      const unsigned vq = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)bq + 4u * (unsigned)(h * 32 + l32);
      unsigned vp[WG_MAXT];
#pragma unroll
      for (int i = 0; i < WG_MAXT; ++i) vp[i] = bpb + 4u * (unsigned)(rowoff[i] + ((h * p.s) << 5));
      // 27 row-tiles over 8 waves: every wave owns tiles w, w+8, w+16 for the whole sub-tile and 1/8 of the voxel pairs
      // of the three left-over tiles 24..26 (its own x-row for stride 1, half a row for stride 2) in a second, short
      // sweep -> 216 MFMAs per wave and sub-tile on every wave instead of 256 / 192 (the barrier waits for the slowest)
      using GX = typename std::conditional<FIXG == 1, WgGeo<1, 16, 1, 1>, WgGeo<2, 4, 1, 1>>::type;   // NS = 8 / 2 steps
      static_assert(GX::NS * WG_WAVES == G::NS, "the left-over tiles' steps must split evenly over the waves");
      const int k0 = wave * GX::NS;                       // first step of this wave's slice (wave-uniform)
      const int r0 = k0 / G::JR, j0 = k0 % G::JR;         // its x-row (z-major) and position inside the row
      const int pb0 = (((r0 >> 2) * p.s * p.IY + (r0 & 3) * p.s) * p.IX + 2 * j0 * p.s) * 128;   // = G::p_b(k0), TY = 4
      unsigned vpx[WG_MAXT];
#pragma unroll
      for (int i = 0; i < 3; ++i) vpx[i] = bpb + 4u * (unsigned)(rowoffx[i] + ((h * p.s) << 5)) + (unsigned)pb0;
      vpx[3] = vpx[2];
      auto nostage = [](auto) {};
      wgrad_sweep_fixed<3, GX>(vpx, vq + (unsigned)(k0 * 256), accx, nostage);
      wgrad_sweep_fixed<3, G>(vp, vq, acc, stage);
    } else {
      const int st0 = ksplit ? wave : 0, stinc = ksplit ? WG_WAVES : 1;
      switch (ntw) {  // wave-uniform: row-tiles this wave owns -> branch-free MFMA bodies
        case 4: wgrad_steps<4>(p, bp, bq, rowoff, acc, st0, stinc, nsteps, h, l32); break;
        case 3: wgrad_steps<3>(p, bp, bq, rowoff, acc, st0, stinc, nsteps, h, l32); break;
        case 2: wgrad_steps<2>(p, bp, bq, rowoff, acc, st0, stinc, nsteps, h, l32); break;
        case 1: wgrad_steps<1>(p, bp, bq, rowoff, acc, st0, stinc, nsteps, h, l32); break;
        default: break;
      }
    }
    if (more) {
      if constexpr (GLDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else commit(lds + (cur ^ 1) * bufDw);
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- write partials ----
  const long tileBase = ((((long)blockIdx.x * gridDim.y + pct) * gridDim.z + qct) * p.ntiles) * 1024;
  if constexpr (FIXG != 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // the wave's own tiles w, w+8, w+16
      float* dst = p.partial + tileBase + (long)(wave + WG_WAVES * i) * 1024;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + l32] = acc[i][r];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // tiles 24..26: fixed-order sum of the 8 waves' K-slices through LDS
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) lds[wave * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + l32] = accx[i][r];
      __syncthreads();
      float* dst = p.partial + tileBase + (long)(24 + i) * 1024;
      for (int e = tid; e < 1024; e += WG_THREADS) {
        float s = lds[e];
#pragma unroll
        for (int w = 1; w < WG_WAVES; ++w) s += lds[w * 1024 + e];
        dst[e] = s;
      }
    }
  } else if (!ksplit) {
#pragma unroll
    for (int i = 0; i < WG_MAXT; ++i) {
      const int tile = wave + WG_WAVES * i;
      if (tile < p.ntiles) {
        float* dst = p.partial + tileBase + (long)tile * 1024;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + l32] = acc[i][r];
      }
    }
  } else {
    // cross-wave fixed-order reduction through LDS (staging buffers are free now)
#pragma unroll
    for (int i = 0; i < WG_MAXT; ++i) {
      if (i < p.ntiles) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) lds[wave * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + l32] = acc[i][r];
        __syncthreads();
        float* dst = p.partial + tileBase + (long)i * 1024;
        for (int e = tid; e < 1024; e += WG_THREADS) {
          float s = lds[e];
#pragma unroll
          for (int w = 1; w < WG_WAVES; ++w) s += lds[w * 1024 + e];
          dst[e] = s;
        }
      }
    }
  }
  if (p.want_bias && pct == 0) {
    __syncthreads();
    double* shd = reinterpret_cast<double*>(lds);
    shd[tid] = bsum;
    __syncthreads();
    if (tid < 32) {
      double s = 0.0;
      for (int part = 0; part < 16; ++part) s += shd[part * 32 + tid];
      p.partial_b[((long)blockIdx.x * gridDim.z + qct) * 32 + tid] = s;
    }
  }
}

struct WfinParams {
  const float* partial;
  const double* partial_b;
  float* dw;
  float* db;
  int nsp, npct, nqct, ntaps, ntiles, cpad, Cp, Cq;
  long sT, sP, sQ;
  int fold_axis;  // 0 none, 1 the P-channel axis is the (possibly folded) reference Cin axis, 2 the Q axis is
  int shift, dup_start;
  int accum;
};

// dW[t][pc][qc] (+)= sum_wg partial.  One block per row (32 consecutive qc of one (t, pc, qct)): 256 threads = 8 float4
// columns x 32 partial-lanes, every lane streams its share of the nsp partials (4 independent 16-byte loads in flight),
// fp64 accumulate, fixed-order combine through LDS (bitwise reproducible).  The pass is pure HBM streaming.
// Folded slab channel c maps to reference channel c+shift and, if c >= dup_start, also to c-dup_start (both copies of
// the duplicated slice see the same input: encoder.py:83-87).
__global__ __launch_bounds__(256) void wgrad_finalize_kernel(const WfinParams f) {
  __shared__ double sh[32][33];
  const int q4 = threadIdx.x & 7, wl = threadIdx.x >> 3;
  const long rows = (long)f.ntaps * f.Cp * f.nqct;
  const long wgStride = (long)f.npct * f.nqct * f.ntiles * 1024;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int qct = (int)(row % f.nqct);
    long r = row / f.nqct;
    const int pc = (int)(r % f.Cp);
    const int t = (int)(r / f.Cp);
    long off;
    if (f.cpad == 32) off = ((((long)(pc >> 5)) * f.nqct + qct) * f.ntiles + t) * 1024 + (pc & 31) * 32;
    else {
      const int ci = t * f.cpad + pc;
      off = ((long)qct * f.ntiles + (ci >> 5)) * 1024 + (ci & 31) * 32;
    }
    const float* src = f.partial + off + q4 * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // fp64 combine of the per-workgroup fp32 partials
    int w = wl;
    for (; w + 96 < f.nsp; w += 128) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + (long)w * wgStride);
      const f32x4 b = *reinterpret_cast<const f32x4*>(src + (long)(w + 32) * wgStride);
      const f32x4 c = *reinterpret_cast<const f32x4*>(src + (long)(w + 64) * wgStride);
      const f32x4 d = *reinterpret_cast<const f32x4*>(src + (long)(w + 96) * wgStride);
      s0 += (double)a[0]; s1 += (double)a[1]; s2 += (double)a[2]; s3 += (double)a[3];
      s0 += (double)b[0]; s1 += (double)b[1]; s2 += (double)b[2]; s3 += (double)b[3];
      s0 += (double)c[0]; s1 += (double)c[1]; s2 += (double)c[2]; s3 += (double)c[3];
      s0 += (double)d[0]; s1 += (double)d[1]; s2 += (double)d[2]; s3 += (double)d[3];
    }
    for (; w < f.nsp; w += 32) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + (long)w * wgStride);
      s0 += (double)a[0]; s1 += (double)a[1]; s2 += (double)a[2]; s3 += (double)a[3];
    }
    __syncthreads();
    sh[wl][q4 * 4 + 0] = s0; sh[wl][q4 * 4 + 1] = s1; sh[wl][q4 * 4 + 2] = s2; sh[wl][q4 * 4 + 3] = s3;
    __syncthreads();
    if (threadIdx.x < 32) {
      const int e = threadIdx.x;
      double totd = sh[0][e];
#pragma unroll
      for (int k = 1; k < 32; ++k) totd += sh[k][e];
      const float tot = (float)totd;
      const int qc = qct * 32 + e;
      if (qc < f.Cq) {
        const int pr = (f.fold_axis == 1) ? pc + f.shift : pc;
        const int qr = (f.fold_axis == 2) ? qc + f.shift : qc;
        float* d1 = f.dw + t * f.sT + pr * f.sP + qr * f.sQ;
        *d1 = f.accum ? (*d1 + tot) : tot;
        if (f.shift > 0) {
          if (f.fold_axis == 1 && pc >= f.dup_start) {
            float* d2 = f.dw + t * f.sT + (pc - f.dup_start) * f.sP + qr * f.sQ;
            *d2 = f.accum ? (*d2 + tot) : tot;
          } else if (f.fold_axis == 2 && qc >= f.dup_start) {
            float* d2 = f.dw + t * f.sT + pr * f.sP + (qc - f.dup_start) * f.sQ;
            *d2 = f.accum ? (*d2 + tot) : tot;
          }
        }
      }
    }
  }
  // bias: block qct combines the per-workgroup fp64 column sums of its 32 channels (32 channels x 8 partial-lanes)
  if (f.db && (int)blockIdx.x < f.nqct) {
    const int e = threadIdx.x & 31, l8 = threadIdx.x >> 5, qct = blockIdx.x;
    double s = 0.0;
    for (int w = l8; w < f.nsp; w += 8) s += f.partial_b[((long)w * f.nqct + qct) * 32 + e];
    __syncthreads();
    sh[l8][e] = s;
    __syncthreads();
    if (l8 == 0 && qct * 32 + e < f.Cq) {
      double tot = sh[0][e];
#pragma unroll
      for (int k = 1; k < 8; ++k) tot += sh[k][e];
      const int i = qct * 32 + e;
      f.db[i] = f.accum ? (f.db[i] + (float)tot) : (float)tot;
    }
  }
}

// Same combine for few partials (nsp <= 16): one thread per output element, partials read coalesced along qc.
__global__ __launch_bounds__(256) void wgrad_finalize_flat_kernel(const WfinParams f) {
  const int nq = f.nqct * 32;
  const long total = (long)f.ntaps * f.Cp * nq;
  const long wgStride = (long)f.npct * f.nqct * f.ntiles * 1024;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int qc = (int)(i % nq);
    long r = i / nq;
    const int pc = (int)(r % f.Cp);
    const int t = (int)(r / f.Cp);
    if (qc >= f.Cq) continue;
    const int qct = qc >> 5, e = qc & 31;
    long off;
    if (f.cpad == 32) off = ((((long)(pc >> 5)) * f.nqct + qct) * f.ntiles + t) * 1024 + (pc & 31) * 32 + e;
    else {
      const int ci = t * f.cpad + pc;
      off = ((long)qct * f.ntiles + (ci >> 5)) * 1024 + (ci & 31) * 32 + e;
    }
    double totd = 0.0;
    for (int w = 0; w < f.nsp; ++w) totd += (double)f.partial[w * wgStride + off];
    const float tot = (float)totd;
    const int pr = (f.fold_axis == 1) ? pc + f.shift : pc;
    const int qr = (f.fold_axis == 2) ? qc + f.shift : qc;
    float* d1 = f.dw + t * f.sT + pr * f.sP + qr * f.sQ;
    *d1 = f.accum ? (*d1 + tot) : tot;
    if (f.shift > 0) {
      if (f.fold_axis == 1 && pc >= f.dup_start) {
        float* d2 = f.dw + t * f.sT + (pc - f.dup_start) * f.sP + qr * f.sQ;
        *d2 = f.accum ? (*d2 + tot) : tot;
      } else if (f.fold_axis == 2 && qc >= f.dup_start) {
        float* d2 = f.dw + t * f.sT + pr * f.sP + (qc - f.dup_start) * f.sQ;
        *d2 = f.accum ? (*d2 + tot) : tot;
      }
    }
  }
  if (f.db && blockIdx.x == 0) {
    for (int i = threadIdx.x; i < f.Cq; i += blockDim.x) {
      double s = 0.0;
      for (int w = 0; w < f.nsp; ++w) s += f.partial_b[((long)w * f.nqct + (i >> 5)) * 32 + (i & 31)];
      f.db[i] = f.accum ? (f.db[i] + (float)s) : (float)s;
    }
  }
}

static int ilog2w(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// ---- ONE choice per call: which kernel takes it, on which grid, and where its workspace areas lie.  wgrad_choose makes it; the
// queries and the launch answer from it ----
struct WgCall {           // kind, shape, strides (elements) and what the operands allow -- no pointers
  int kind;
  int N, D, H, W;         // the forward INPUT dims
  int Cin, ldx, Cout, lddy;      // Cin: the slab (folded) count
  int dup_shift;
  int want_db;
  int x16, dy16;          // x / dy on a 16-byte boundary
};
struct WgradRoles {
  int ntaps, s, neg, swapped, transposed;
  int Dp, Hp, Wp, Cp, Dq, Hq, Wq, Cq;
};
struct WgChoice {
  WgradRoles ro;
  WgradParams p;          // as planned, without its pointers
  int nsp, npct, nqct;
  size_t shmem;
  int variant;            // staging of wgrad_kernel: 0 register | 1 LDS-DMA | 2, 3 the fixed-geometry sweeps (stride 1, 2)
  int sym;                // profile symbol of the kernel that runs: 100 | 104 | 109 | 110 wgrad_kernel of `variant` (100 + (MODE << 2 | FIXG)) |
                          // 24 wgw_kernel | 26 k1w_kernel
  long NV;                // voxels of Q: the contraction length
  double flops;           // what the launch is profiled with
  int clear_zeros;        // the kernel reads the zero tail: the padding lanes of the general LDS-DMA staging (104) only
  // workspace, byte offsets: partials | bias partials | column sums of dy (swapped form's db; colsum_bytes of them) | 64 zero bytes; ws: all
  long ws_partial, ws_partial_b, ws_colsum, colsum_bytes, ws_zeros, ws;
};

// Tiling and K-split of the roles: pl.p (no pointers, no strides), nsp / npct / nqct, shmem.  neg: tap offsets are negated (swapped-role
// form, s == 1 only)
static int plan_wgrad(WgChoice& pl, int ntaps, int s, int neg, int N, int Dp, int Hp, int Wp_, int Cp, int Dq, int Hq,
                      int Wq, int Cq) {
  WgradParams& p = pl.p;
  p.N = N; p.Dp = Dp; p.Hp = Hp; p.Wp = Wp_; p.Cp = Cp;
  p.Dq = Dq; p.Hq = Hq; p.Wq = Wq; p.Cq = Cq;
  p.s = s; p.ntaps = ntaps;
  int lo = 0, span = 1;
  if (ntaps == 27 && s == 1) { lo = -1; span = 3; }
  if (ntaps == 27 && s == 2) { lo = 0; span = 3; }
  p.loz = p.loy = p.lox = lo;
  // (tap, channel) row packing when P has few channels
  int cpad = 32;
  if (Cp <= 16 && ntaps == 27) { cpad = 2; while (cpad < Cp) cpad *= 2; }
  p.cpad = cpad;
  const int SP = cpad == 32 ? 32 : (cpad < 4 ? 4 : cpad);
  p.lgSP = ilog2w(SP);
  p.ntiles = (cpad == 32) ? ntaps : (ntaps * cpad + 31) / 32;
  // sub-tile: 128 voxels for s=1 (16x4x2), 32 voxels for s=2 (8x4x1); 1x1x1: 256 voxels (32x4x2)
  int TX, TY, TZ;
  if (ntaps == 1) { TX = 32; TY = 4; TZ = 2; }
  else if (s == 1) { TX = 16; TY = 4; TZ = 2; }
  else { TX = 8; TY = 4; TZ = 1; }
  while (TX > 2 && TX / 2 >= Wq) { TX /= 2; if (TY * 2 <= 8) TY *= 2; else TZ *= 2; }
  while (TY > 1 && TY / 2 >= Hq) { TY /= 2; TZ *= 2; }
  while (TZ > 1 && TZ / 2 >= Dq && TX * TY * (TZ / 2) >= 2) TZ /= 2;
  p.lgTX = ilog2w(TX); p.lgTY = ilog2w(TY); p.TZ = TZ;
  p.ntx = (Wq + TX - 1) / TX; p.nty = (Hq + TY - 1) / TY; p.ntz = (Dq + TZ - 1) / TZ;
  p.IX = (TX - 1) * s + span; p.IY = (TY - 1) * s + span; p.IZ = (TZ - 1) * s + span;
  const int tileVoxP = p.IZ * p.IY * p.IX;
  const int M = TX * TY * TZ;
  if (tileVoxP * (SP / 4) > WG_THREADS * WG_PSLOTS || M * 8 > WG_THREADS * WG_QSLOTS) return BTS_ERR_SHAPE;
  pl.shmem = (size_t)2 * ((((tileVoxP * (SP / 4) + 63) & ~63) + ((M * 8 + 63) & ~63)) * 4) * sizeof(float);
  if (pl.shmem < (size_t)WG_WAVES * 1024 * sizeof(float)) pl.shmem = (size_t)WG_WAVES * 1024 * sizeof(float);
  if (pl.shmem > 160 * 1024) return BTS_ERR_SHAPE;
  for (int t = 0; t < 27; ++t) p.tap_vox[t] = 0;
  if (ntaps == 27)
    for (int t = 0; t < 27; ++t) {
      int oz = t / 9 + (s == 1 ? -1 : 0), oy = (t / 3) % 3 + (s == 1 ? -1 : 0), ox = t % 3 + (s == 1 ? -1 : 0);
      if (neg) { oz = -oz; oy = -oy; ox = -ox; }
      p.tap_vox[t] = ((oz - lo) * p.IY + (oy - lo)) * p.IX + (ox - lo);
    }
  p.fixg = 0;
  if (ntaps == 27 && cpad == 32 && !neg) {
    if (s == 1 && TX == 16 && TY == 4 && TZ == 2) p.fixg = 1;
    if (s == 2 && TX == 8 && TY == 4 && TZ == 1) p.fixg = 2;
  }
  p.fastf = 0;
  if (p.fixg && Wq % TX == 0 && Hq % TY == 0 && Dq % TZ == 0 && Cp % 32 == 0 && Cq % 32 == 0)
    p.fastf = 1;  // (the 32-bit staging offsets are range-checked where the leading dimensions are known)
  if (!p.fastf) p.fixg = 0;  // the fixed sweep only ships together with the fast staging
  p.nsub = N * p.ntz * p.nty * p.ntx;
  pl.npct = (cpad == 32) ? (Cp + 31) / 32 : 1;
  pl.nqct = (Cq + 31) / 32;
  // K-split count nsp (workgroups per (P,Q) channel-tile pair).  One workgroup is resident per CU, so the launch runs in
  // rounds of 256; cost model in units of one sub-tile sweep: rounds x (sub-tiles per WG + 0.5 fixed) + the partials'
  // write/combine traffic (~0.0023 per workgroup).  Smallest cost wins, ties go to fewer partials.
  {
    const long pairs = (long)pl.npct * pl.nqct;
    long best = 1;
    double bestc = 1e30;
    long maxn = 2048 / pairs;
    if (maxn < 1) maxn = 1;
    if (maxn > p.nsub) maxn = p.nsub;
    for (long n = 1; n <= maxn; ++n) {
      const long spw = (p.nsub + n - 1) / n;
      const long ne = (p.nsub + spw - 1) / spw;
      if (ne != n) continue;
      const long rounds = (ne * pairs + 255) / 256;
      const double c = (double)rounds * ((double)spw + 0.5) + 0.0023 * (double)(ne * pairs);
      if (c < bestc - 1e-9) { bestc = c; best = n; }
    }
    if (best > p.nsub) best = p.nsub;
    p.sub_per_wg = (int)((p.nsub + best - 1) / best);
    pl.nsp = (p.nsub + p.sub_per_wg - 1) / p.sub_per_wg;
  }
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient of the 3x3x3 stride-1 convolution in Winograd form with all three axes transformed, F(2x2x2, 3x3x3) -- the
// counterpart of conv_wino3.hip for  dW[kz,ky,kx,c,k] = sum_v P[v + (kz-1,ky-1,kx-1)][c] * Q[v][k]:
//   dW = (G^T x G^T x G^T) sum over 2x2x2 patches of  [ (B^T x B^T x B^T) P_4x4x4 ] o [ (A x A x A) Q_2x2x2 ]
// (B^T, G, A^T as in conv_wino3.hip's header; P = x with a one-voxel halo, Q = dy).  64 accumulator tiles, each fed one
// patch = 8 voxels at a time: 8/27 of the direct form's matrix instructions.  The contraction runs over patches, so channels
// sit on the lanes.  4 waves = the 4 xi_z, each 16 accumulators (xi_y, xi_x) = 256 registers, one wave per SIMD.
// Lane = (channel, patch parity): the K = 2 of an instruction is two x-neighbouring patches, so the sub-tile 16 x 4 x 2 = 16
// patches (the direct kernel's: plan, partial layout [27 taps][32][32] per workgroup and finalize kernels are shared) is 8 steps
// of 16 matrix instructions.  LDS tiles are x-fastest, [row][channel][18], transposed while staging: P rows hold x = -1..16, Q
// rows x = 0..15 (+2 unused).  A lane's four x inputs of a patch are two 8-byte reads at an 8-byte-aligned offset; the row
// stride of 18 floats sends the 32 channels of a half wave to 32 distinct bank pairs ((9 c) mod 32 is a permutation):
// conflict-free.  Staging slots run channel quad fastest, then x: a wave's 16-byte loads are contiguous in memory and its
// transposing 4-byte LDS writes hit banks 8 cq + x (8 x 8 distinct).  The z combination of P is taken on the way into LDS, as
// w3_kernel's commit() does: a thread stages the four z rows of one column and writes the planes d0 - d2 | d1 + d2 | d2 - d1 |
// d1 - d3 into the rows of the four z rows, a wave reads the plane of its own xi_z and transforms y and x.  Q stays raw (its
// planes would not fit); xi = 3 of Q carries +q1 for the true -q1 on every axis, undone where G^T is applied (in the wave for y
// and x, across the waves through LDS for z).  Every step is branch-free: the next sub-tile's loads go through descriptors that
// are empty behind the workgroup's last sub-tile, and everything a step consumes was asked for two steps earlier (global loads
// before their LDS writes, LDS reads before their matrix instructions).  Bias partials: the all-sum point of Q (xi = 1 on every
// axis, wave 1).
// ---------------------------------------------------------------------------------------------------------------------
typedef float wg_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wg_f32x2 wgw_pk_add(wg_f32x2 a, wg_f32x2 b) { wg_f32x2 d; asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ wg_f32x2 wgw_pk_sub(wg_f32x2 a, wg_f32x2 b) { wg_f32x2 d; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ wg_f32x2 wgw_pk_fma(wg_f32x2 a, wg_f32x2 b, wg_f32x2 c) { wg_f32x2 d; asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
// (a.x + b.y, a.x - b.y)
__device__ __forceinline__ wg_f32x2 wgw_pk_addsub(wg_f32x2 a, wg_f32x2 b) { wg_f32x2 d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ float wgw_acc_rd(float a) { float v; asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a)); return v; }

#define WGW_THREADS 256
#define WGW_RS 18
#define WGW_PTILE (24 * 32 * WGW_RS)         /* 4 z-rows x 6 y-rows */
#define WGW_QTILE (8 * 32 * WGW_RS)          /* 2 z-rows x 4 y-rows */
#define WGW_BUF (WGW_PTILE + WGW_QTILE)      /* 18432 floats = 72 KB, double buffered; the two = the 4 x 9 tiles of the combine */
#define WGW_PLANE (6 * 32 * WGW_RS)          /* one xi_z plane of the P tile: 6 y-rows */
#define WGW_NPC 4                            /* P column slots per thread: 6 y-rows x 18 x x 8 channel quads = 864 = 3.375 x 256 */
#define WGW_NQS 4                            /* Q slots per thread: 8 rows x 16 x x 8 channel quads = 1024 */

__global__ __launch_bounds__(WGW_THREADS, 1) void wgw_kernel(const WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // = xi_z
  const int ch = lane & 31, hh = lane >> 5;
  const int pct = blockIdx.y, qct = blockIdx.z;
  const float* pP = p.p + pct * 32;
  const float* pQ = p.q + qct * 32;

  // ---- staging maps.  P: column id = tid + 256*i = ((y row * 18) + x) * 8 + channel quad; a thread loads the four z rows of its
  //      column, each through the descriptor of that z row, and writes the four xi_z planes.  Byte offsets relative to the z row's
  //      origin are computed once; a column on a y or x face of the image gets a 2 GB offset = outside the descriptor, the load
  //      returns zeros (4 face bits per column against 4 per tile); a z row outside the image has an empty descriptor.
  //      Q: slot id = tid + 256*i = ((row * 16) + x) * 8 + channel quad, raw. ----
  int c_lds[WGW_NPC - 1], c3_lds[4];
  unsigned coff[WGW_NPC], cfl = 0u;
#pragma unroll
  for (int i = 0; i < WGW_NPC; ++i) {
    const int id = tid + WGW_THREADS * i;
    int l = 0;
    coff[i] = 0x80000000u;
    if (id < 6 * 18 * 8) {
      const int cq = id & 7, vox = id >> 3;
      const int yr = vox / 18, xx = vox - yr * 18;
      l = (yr * 32 + cq * 4) * WGW_RS + xx;
      coff[i] = (unsigned)((yr * p.Wp + xx) * p.ldp + cq * 4) * 4u;
      const unsigned fl = (yr == 0 ? 1u : 0u) | (yr == 5 ? 2u : 0u) | (xx == 0 ? 4u : 0u) | (xx == 17 ? 8u : 0u);
      cfl |= fl << (4 * i);
    }
    if (i < WGW_NPC - 1) {
      c_lds[i < WGW_NPC - 1 ? i : 0] = l;
    } else {
      // (the partly filled last slot: its idle threads load nothing and write their zeros to the unused x = 16, 17 of the Q rows,
      // four channels of one row per plane)
      const int idle = id - 6 * 18 * 8;
#pragma unroll
      for (int pl = 0; pl < 4; ++pl)
        c3_lds[pl] = idle < 0 ? l + pl * WGW_PLANE : WGW_PTILE + 4 * (((idle >> 1) + 16 * pl) & 63) * WGW_RS + 16 + (idle & 1);
    }
  }
  int q_lds[WGW_NQS];
  unsigned qoff[WGW_NQS];
#pragma unroll
  for (int i = 0; i < WGW_NQS; ++i) {
    const int id = tid + WGW_THREADS * i;
    const int cq = id & 7, xx = (id >> 3) & 15, row = id >> 7;   // row = oz*4 + oy
    q_lds[i] = WGW_PTILE + (row * 32 + cq * 4) * WGW_RS + xx;
    qoff[i] = (unsigned)((((row >> 2) * p.Hq + (row & 3)) * p.Wq + xx) * p.ldq + cq * 4) * 4u;
  }
  const int t0 = blockIdx.x * p.sub_per_wg;
  int t1 = t0 + p.sub_per_wg;
  if (t1 > p.nsub) t1 = p.nsub;
  // coordinates and origins (P: the halo corner) of the NEXT sub-tile to fetch.  Sub-tiles of a workgroup are consecutive: the
  // coordinates advance by carries and the origins by 32-bit byte strides, no division or 64-bit product in the loop
  int ftx, fty, ftz, fn;
  {
    int t = t0;
    ftx = t % p.ntx; t /= p.ntx;
    fty = t % p.nty; t /= p.nty;
    ftz = t % p.ntz;
    fn = t / p.ntz;
  }
  const char* f_pb = reinterpret_cast<const char*>(pP + ((((long)fn * p.Dp + 2 * ftz - 1) * p.Hp + 4 * fty - 1) * p.Wp + 16 * ftx - 1) * p.ldp);
  const char* f_qb = reinterpret_cast<const char*>(pQ + ((((long)fn * p.Dq + 2 * ftz) * p.Hq + 4 * fty) * p.Wq + 16 * ftx) * p.ldq);
  const long zrow = (long)p.Hp * p.Wp * p.ldp;
  // bytes to the next sub-tile along x; more to the first of the next y row; more to the first of the next z row (tiles are whole
  // and samples contiguous: the next sample's first is one more z row on).  The launcher keeps five z rows of P and three of Q
  // below 2 GB.
  const unsigned pdx = 64u * p.ldp, pdy = 12u * p.Wp * p.ldp, pdz = (unsigned)zrow * 4u;
  const unsigned qdx = 64u * p.ldq, qdy = 12u * p.Wq * p.ldq, qdz = (unsigned)p.Hq * p.Wq * p.ldq * 4u;
  // The 20 requests of the next sub-tile go out in six groups (P column 0 | 1 | 2 | 3, four z rows each | Q 0-1 | Q 2-3).  Group k is
  // written to the OTHER LDS buffer at step k and requested two steps before that -- groups 0 and 1 in the last two steps of the
  // sub-tile before, where fetch_begin has just made its descriptors: a request has two steps to come back before the in-order
  // wait of its write.
  f32x4 pre[4 * WGW_NPC + WGW_NQS];
  __amdgpu_buffer_rsrc_t f_pr[4], f_qr;
  unsigned f_cm[WGW_NPC] = {0u, 0u, 0u, 0u};   // the tile's y / x face bits at the place of each column's
  auto fetch_begin = [&](bool live) {   // live = false: empty descriptors, every load returns zeros without traffic
    const float* pb = reinterpret_cast<const float*>(f_pb);
    const float* qb = reinterpret_cast<const float*>(f_qb);
    f_pr[0] = __builtin_amdgcn_make_buffer_rsrc((void*)pb, 0, (live && ftz != 0) ? 0x7fffffff : 0, 0x00020000);
    f_pr[1] = __builtin_amdgcn_make_buffer_rsrc((void*)(pb + zrow), 0, live ? 0x7fffffff : 0, 0x00020000);
    f_pr[2] = __builtin_amdgcn_make_buffer_rsrc((void*)(pb + 2 * zrow), 0, live ? 0x7fffffff : 0, 0x00020000);
    f_pr[3] = __builtin_amdgcn_make_buffer_rsrc((void*)(pb + 3 * zrow), 0, (live && ftz != p.ntz - 1) ? 0x7fffffff : 0, 0x00020000);
    f_qr = __builtin_amdgcn_make_buffer_rsrc((void*)qb, 0, live ? 0x7fffffff : 0, 0x00020000);
    const unsigned tm = (fty == 0 ? 1u : 0u) | (fty == p.nty - 1 ? 2u : 0u) | (ftx == 0 ? 4u : 0u) | (ftx == p.ntx - 1 ? 8u : 0u);
#pragma unroll
    for (int i = 0; i < WGW_NPC; ++i) f_cm[i] = tm << (4 * i);
    const int cx = (ftx + 1 == p.ntx) ? 1 : 0;   // (selects, no branches: the call sits inside a scheduled step)
    ftx = cx ? 0 : ftx + 1;
    const int cy = (fty + cx == p.nty) ? 1 : 0;
    fty = cy ? 0 : fty + cx;
    const int cz = (ftz + cy == p.ntz) ? 1 : 0;
    ftz = cz ? 0 : ftz + cy;
    f_pb += pdx + cx * pdy + cy * pdz;   // (cy implies cx)
    f_qb += qdx + cx * qdy + cy * qdz;
  };
  auto load4 = [](__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
  };
  auto sub4 = [](f32x4 a, f32x4 b) {
    const wg_f32x2 lo = wgw_pk_sub(a.xy, b.xy), hi = wgw_pk_sub(a.zw, b.zw);
    return f32x4{lo.x, lo.y, hi.x, hi.y};
  };
  auto add4 = [](f32x4 a, f32x4 b) {
    const wg_f32x2 lo = wgw_pk_add(a.xy, b.xy), hi = wgw_pk_add(a.zw, b.zw);
    return f32x4{lo.x, lo.y, hi.x, hi.y};
  };
  auto fetch_group = [&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if constexpr (k < WGW_NPC) {
      const unsigned off = (cfl & f_cm[k]) ? 0x80000000u : coff[k];
#pragma unroll
      for (int zr = 0; zr < 4; ++zr) pre[4 * k + zr] = load4(f_pr[zr], off);
    } else {
      constexpr int i = 2 * (k - WGW_NPC);
      pre[4 * WGW_NPC + i] = load4(f_qr, qoff[i]);
      pre[4 * WGW_NPC + i + 1] = load4(f_qr, qoff[i + 1]);
    }
  };
  auto commit_group = [&](float* buf, auto kc) {
    constexpr int k = decltype(kc)::value;
    if constexpr (k < WGW_NPC) {   // xi_z planes d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3 of the column, into the rows of the four z rows
      const f32x4 d0 = pre[4 * k], d1 = pre[4 * k + 1], d2 = pre[4 * k + 2], d3 = pre[4 * k + 3];
      const f32x4 pl[4] = {sub4(d0, d2), add4(d1, d2), sub4(d2, d1), sub4(d1, d3)};
#pragma unroll
      for (int z = 0; z < 4; ++z) {
        float* o;
        if constexpr (k < WGW_NPC - 1) o = buf + c_lds[k] + z * WGW_PLANE;
        else o = buf + c3_lds[z];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e * WGW_RS] = pl[z][e];
      }
    } else {
      constexpr int i0 = 2 * (k - WGW_NPC);
#pragma unroll
      for (int i = i0; i < i0 + 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) buf[q_lds[i] + e * WGW_RS] = pre[4 * WGW_NPC + i][e];
    }
  };
  // the staging share of step s: write group s (steps 0-5: the barrier sits before step 6), request the group that is written two
  // steps on.  The descriptors of the sub-tile after the next (live2: it exists) are made in step 6, which requests its group 0,
  // behind the last request of the next (group 5, step 3)
  auto stage = [&](float* buf, auto sc, bool live2) {
    constexpr int s = decltype(sc)::value;
    if constexpr (s <= 5) commit_group(buf, IC<s>{});
    if constexpr (s == 6) fetch_begin(live2);
    if constexpr (s + 2 <= 5) fetch_group(IC<s + 2>{});
    else if constexpr (s >= 6) fetch_group(IC<s - 6>{});
  };

  // ---- wave roles: xi_z of P: the wave's own plane; of Q: a = X + sq * Y (xi_z = 3: +q1) ----
  const float sq = (wave == 1) ? 1.f : (wave == 2) ? -1.f : 0.f;
  const wg_f32x2 sq2 = {sq, sq};
  const int pA = wave * WGW_PLANE + ch * WGW_RS + 2 * hh;
  const int qXa = WGW_PTILE + ((wave == 3 ? 4 : 0) * 32 + ch) * WGW_RS + 2 * hh;
  const int qYa = WGW_PTILE + (4 * 32 + ch) * WGW_RS + 2 * hh;
  const bool bias = p.want_bias && pct == 0 && wave == 1;
  double bsum = 0.0;
  float bs = 0.f;   // the all-sum point of Q (xi = 1 on every axis; wave 1) over one sub-tile

  f32x16 acc[4][4];   // [xi_y][xi_x]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

  struct WgwOps { float v[4][4], t[4][4]; };
  struct WgwRaw { wg_f32x2 pl[4], px[4], qx[2], qy[2]; };
  // LDS reads of step st = (patch row py, x patch pair sx): this lane's patch is px = 2 sx + hh.  They are issued two steps before
  // the matrix instructions that use them and transformed one step before: a read has a whole step to come back
  auto rd = [&](const float* cur, auto stc, WgwRaw& r) {
    constexpr int st = decltype(stc)::value;
    constexpr int py = st >> 2, sx = st & 3;
#pragma unroll
    for (int yr = 0; yr < 4; ++yr) {   // rows of the wave's xi_z plane: x inputs 0,1 | 2,3
      const float* a = cur + pA + (2 * py + yr) * 32 * WGW_RS + 4 * sx;
      r.pl[yr] = *reinterpret_cast<const wg_f32x2*>(a);
      r.px[yr] = *reinterpret_cast<const wg_f32x2*>(a + 2);
    }
#pragma unroll
    for (int yr = 0; yr < 2; ++yr) {
      r.qx[yr] = *reinterpret_cast<const wg_f32x2*>(cur + qXa + (2 * py + yr) * 32 * WGW_RS + 4 * sx);
      r.qy[yr] = *reinterpret_cast<const wg_f32x2*>(cur + qYa + (2 * py + yr) * 32 * WGW_RS + 4 * sx);
    }
  };
  auto xf = [&](const WgwRaw& r, WgwOps& o) {
    wg_f32x2 vl[4], vx[4];
    vl[0] = wgw_pk_sub(r.pl[0], r.pl[2]); vx[0] = wgw_pk_sub(r.px[0], r.px[2]);
    vl[1] = wgw_pk_add(r.pl[1], r.pl[2]); vx[1] = wgw_pk_add(r.px[1], r.px[2]);
    vl[2] = wgw_pk_sub(r.pl[2], r.pl[1]); vx[2] = wgw_pk_sub(r.px[2], r.px[1]);
    vl[3] = wgw_pk_sub(r.pl[1], r.pl[3]); vx[3] = wgw_pk_sub(r.px[1], r.px[3]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {   // x: e0 - e2 | e1 + e2 | e2 - e1 | e1 - e3
      const wg_f32x2 d = wgw_pk_sub(vl[a], vx[a]), m = wgw_pk_addsub(vx[a], vl[a]);
      o.v[a][0] = d.x;
      o.v[a][1] = m.x;
      o.v[a][2] = m.y;
      o.v[a][3] = d.y;
    }
    const wg_f32x2 qa[2] = {wgw_pk_fma(r.qy[0], sq2, r.qx[0]), wgw_pk_fma(r.qy[1], sq2, r.qx[1])};
    const wg_f32x2 ty[4] = {qa[0], wgw_pk_add(qa[0], qa[1]), wgw_pk_sub(qa[0], qa[1]), qa[1]};
#pragma unroll
    for (int a = 0; a < 4; ++a) {   // x: e0 | e0 + e1 | e0 - e1 | + e1
      const wg_f32x2 m = wgw_pk_addsub(ty[a], ty[a]);
      o.t[a][0] = ty[a].x;
      o.t[a][1] = m.x;
      o.t[a][2] = m.y;
      o.t[a][3] = ty[a].y;
    }
    bs += o.t[1][1];
  };
  auto mfma16 = [&](const WgwOps& o) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.v[a][b], o.t[a][b], acc[a][b], 0, 0, 0);
  };
  // one slot of the schedule per matrix instruction: the MFMA, then up to four vector-ALU operations and three memory operations
  // of the work that shares the step (next step's operands, the staging group)
#define WGW_SCHED_STEP()                                   \
  _Pragma("unroll") for (int q_ = 0; q_ < 16; ++q_) {      \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     \
    __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);     \
    __builtin_amdgcn_sched_group_barrier(0x320, 3, 0);     \
  }
#define WGW_STEP_END()                       \
  WGW_SCHED_STEP();                          \
  __builtin_amdgcn_sched_barrier(0);         \
  asm volatile("s_nop 1" ::: "memory");   /* hand-written VALU -> MFMA operand: the compiler does not track that hazard */

  fetch_begin(t0 < t1);
  fetch_group(IC<0>{}); fetch_group(IC<1>{}); fetch_group(IC<2>{}); fetch_group(IC<3>{}); fetch_group(IC<4>{}); fetch_group(IC<5>{});
  commit_group(lds, IC<0>{}); commit_group(lds, IC<1>{}); commit_group(lds, IC<2>{}); commit_group(lds, IC<3>{});
  commit_group(lds, IC<4>{}); commit_group(lds, IC<5>{});
  __syncthreads();
  WgwOps opA, opB;
  WgwRaw rawA, rawB;
  // (in the order of the loop's last two steps, so that the waits counted behind the loop's head are the same on both ways in)
  rd(lds, IC<0>{}, rawA);
  __builtin_amdgcn_sched_barrier(0);
  fetch_begin((t0 + 1) < t1);
  fetch_group(IC<0>{});
  __builtin_amdgcn_sched_barrier(0);
  rd(lds, IC<1>{}, rawB);
  __builtin_amdgcn_sched_barrier(0);
  xf(rawA, opA);
  __builtin_amdgcn_sched_barrier(0);
  fetch_group(IC<1>{});
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 3" ::: "memory");
  // step s: the matrix instructions of step s, the transform of step s + 1, the LDS reads of step s + 2, the staging share
  for (int t = t0; t < t1; ++t) {
    const float* cur = lds + ((t - t0) & 1) * WGW_BUF;
    float* nxt = lds + ((t - t0 + 1) & 1) * WGW_BUF;
    const bool live2 = (t + 2) < t1;
    rd(cur, IC<2>{}, rawA); xf(rawB, opB); stage(nxt, IC<0>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    rd(cur, IC<3>{}, rawB); xf(rawA, opA); stage(nxt, IC<1>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
    rd(cur, IC<4>{}, rawA); xf(rawB, opB); stage(nxt, IC<2>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    rd(cur, IC<5>{}, rawB); xf(rawA, opA); stage(nxt, IC<3>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
    rd(cur, IC<6>{}, rawA); xf(rawB, opB); stage(nxt, IC<4>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    rd(cur, IC<7>{}, rawB); xf(rawA, opA); stage(nxt, IC<5>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
    // the barrier sits before step 6: the reads of the next sub-tile's steps 0 and 1 go out under this sub-tile's last two steps and
    // its step 0 is formed under the last (behind the workgroup's last sub-tile the other buffer holds zeros or stale data and
    // what is formed from it is dropped)
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    rd(nxt, IC<0>{}, rawA); xf(rawB, opB); stage(nxt, IC<6>{}, live2);
    mfma16(opA);
    WGW_STEP_END();
    bsum += (double)bs;   // (step 0's share is added when it is formed, under the last step)
    bs = 0.f;
    rd(nxt, IC<1>{}, rawB); xf(rawA, opA); stage(nxt, IC<7>{}, live2);
    mfma16(opB);
    WGW_STEP_END();
  }

  // ---- G^T dU G: y and x part in the wave (xi = 3 carries the opposite sign) -> LDS [xi_z][ky*3+kx][c][k]; z part across the waves ----
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
  __syncthreads();   // (the last step formed operands from the other buffer)
  float* xl = lds + wave * 9 * 1024;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float m[3][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float u0 = wgw_acc_rd(acc[0][b][r]), u1 = wgw_acc_rd(acc[1][b][r]), u2 = wgw_acc_rd(acc[2][b][r]),
                  u3 = wgw_acc_rd(acc[3][b][r]);
      const float hs = 0.5f * (u1 + u2), hd = 0.5f * (u1 - u2);
      m[0][b] = u0 + hs;
      m[1][b] = hd;
      m[2][b] = hs - u3;
    }
    const int crow = 8 * (r >> 2) + 4 * hh + (r & 3);
    float* o = xl + crow * 32 + ch;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const float hs = 0.5f * (m[ky][1] + m[ky][2]), hd = 0.5f * (m[ky][1] - m[ky][2]);
      o[(ky * 3 + 0) * 1024] = m[ky][0] + hs;
      o[(ky * 3 + 1) * 1024] = hd;
      o[(ky * 3 + 2) * 1024] = hs - m[ky][3];
    }
  }
  __syncthreads();
  // taps (kz, ky, kx): kz 0: L0 + .5 L1 + .5 L2 | kz 1: .5 L1 - .5 L2 | kz 2: .5 L1 + .5 L2 - L3   (L3 accumulated with +q1)
  float* out = p.partial + ((((long)blockIdx.x * gridDim.y + pct) * gridDim.z + qct) * 27) * 1024;
  for (int e = tid; e < 9 * 1024; e += WGW_THREADS) {
    const float l0 = lds[0 * 9 * 1024 + e], l1 = lds[1 * 9 * 1024 + e], l2 = lds[2 * 9 * 1024 + e], l3 = lds[3 * 9 * 1024 + e];
    const float hs = 0.5f * (l1 + l2), hd = 0.5f * (l1 - l2);
    out[0 * 9 * 1024 + e] = l0 + hs;   // e = (ky*3 + kx) * 1024 + c * 32 + k
    out[1 * 9 * 1024 + e] = hd;
    out[2 * 9 * 1024 + e] = hs - l3;
  }
  if (bias) {
    const double o = __shfl_xor(bsum, 32, 64);   // the two patch parities of the wave
    if (lane < 32) p.partial_b[((long)blockIdx.x * gridDim.z + qct) * 32 + ch] = bsum + o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient of the 1x1x1 convs (the ResNet blocks' shortcut convs, resnet.py:96-103, and the decoder / VAE projections):
// dW[c][k] = sum_v P[v][c] * Q[v][k] -- a 32x32 tile per (P, Q) channel-group pair with K = all voxels: 2 FLOP per loaded
// byte, HBM-bound.  The staged kernel (LDS DMA, a barrier per 256-voxel sub-tile, 8 matrix instructions between barriers) ran
// these at ~2 TB/s.  Here nothing is staged: the MFMA operand layout (lane = channel, register = voxel of the K pair) is
// exactly a coalesced 128-byte row read, so each lane streams its channel of consecutive voxels with 16 independent 4-byte
// loads in flight and feeds them to the matrix pipe directly; 8 waves per workgroup split the workgroup's voxel range and
// are summed in LDS in fixed order.  Bias partials (column sums of Q) fall out of the B operands.
// ---------------------------------------------------------------------------------------------------------------------
#define K1W_THREADS 512
#define K1W_U 8
__global__ __launch_bounds__(K1W_THREADS, 2) void k1w_kernel(const WgradParams p, long NV, long chunk) {
  __shared__ float lds[8 * 1024];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch = lane & 31, hh = lane >> 5;
  const int pct = blockIdx.y, qct = blockIdx.z;
  const int pc = pct * 32 + ch, qc = qct * 32 + ch;
  const bool pok = pc < p.Cp, qok = qc < p.Cq;
  const long w0 = (long)blockIdx.x * chunk;
  long w1 = w0 + chunk;
  if (w1 > NV) w1 = NV;
  // this wave's part of the workgroup range, whole K pairs
  long per = ((w1 - w0 + 7) / 8 + 1) & ~1L;
  long v = w0 + wave * per;
  long ve = v + per;
  if (ve > w1) ve = w1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  double bsum = 0.0;
  const bool bias = p.want_bias && pct == 0;
  const float* pp = p.p + pc;
  const float* qq = p.q + qc;
  for (; v < ve; v += 2 * K1W_U) {
    float a[K1W_U], b[K1W_U];
#pragma unroll
    for (int u = 0; u < K1W_U; ++u) {
      const long vv = v + 2 * u + hh;
      const bool in = vv < ve;
      a[u] = (in && pok) ? pp[vv * p.ldp] : 0.f;
      b[u] = (in && qok) ? qq[vv * p.ldq] : 0.f;
    }
    float bs = 0.f;
#pragma unroll
    for (int u = 0; u < K1W_U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
      bs += b[u];
    }
    if (bias) bsum += (double)bs;
  }
  // fixed-order sum of the 8 waves' tiles
#pragma unroll
  for (int r = 0; r < 16; ++r) lds[wave * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * hh) * 32 + ch] = acc[r];
  __syncthreads();
  float* dst = p.partial + ((((long)blockIdx.x * gridDim.y + pct) * gridDim.z + qct) * p.ntiles) * 1024;
  for (int e = tid; e < 1024; e += K1W_THREADS) {
    float sacc = lds[e];
#pragma unroll
    for (int w = 1; w < 8; ++w) sacc += lds[w * 1024 + e];
    dst[e] = sacc;
  }
  if (bias) {
    __syncthreads();
    double* shd = reinterpret_cast<double*>(lds);
    shd[tid] = bsum;   // [wave][hh][ch]
    __syncthreads();
    if (tid < 32) {
      double t = 0.0;
      for (int k = 0; k < 16; ++k) t += shd[k * 32 + tid];
      p.partial_b[((long)blockIdx.x * gridDim.z + qct) * 32 + tid] = t;
    }
  }
}

static int wgrad_roles(WgradRoles& r, int kind, int D, int H, int W, int Cin, int Cout) {
  r.ntaps = (kind == BTS_CONV_K1) ? 1 : 27;
  r.s = 1; r.neg = 0; r.swapped = 0; r.transposed = 0;
  r.Dp = D; r.Hp = H; r.Wp = W; r.Cp = Cin; r.Dq = D; r.Hq = H; r.Wq = W; r.Cq = Cout;
  if (kind == BTS_CONV_K3S2) {
    if ((D | H | W) & 1) return BTS_ERR_SHAPE;
    r.s = 2; r.Dq = D / 2; r.Hq = H / 2; r.Wq = W / 2;
  } else if (kind == BTS_CONV_K3S2T) {  // P = dy on the fine grid (2D), Q = x on the coarse grid
    r.transposed = 1;
    r.s = 2; r.Dp = 2 * D; r.Hp = 2 * H; r.Wp = 2 * W; r.Cp = Cout; r.Cq = Cin;
  } else if (kind == BTS_CONV_K3S1 && Cout <= 8 && Cin > Cout) {
    r.swapped = 1; r.neg = 1; r.Cp = Cout; r.Cq = Cin;  // P = dy (tiny), Q = x
  }
  return BTS_OK;
}

extern "C" int bts_colsum(const float* x, float* out, void* workspace, long workspace_bytes, int N, long rows, int C,
                          int ld, float scale, int sum_over_n, int accumulate, hipStream_t stream);
extern "C" long bts_colsum_workspace(int N, long rows, int C);

static bool wg_switch_on(const char* name) {      // (read per call: tests and A/B runs toggle them)
  const char* e = getenv(name);
  return !(e && atoi(e) == 0);
}

// The status bts_conv3d_bwd_weight returns for the call before it looks at its workspace, and for BTS_OK the choice.
static int wgrad_choose(const WgCall& c, WgChoice& ch) {
  WgradRoles& ro = ch.ro;
  int r = wgrad_roles(ro, c.kind, c.D, c.H, c.W, c.Cin, c.Cout);
  if (r != BTS_OK) return r;
  if (c.dup_shift > 0 && (c.kind == BTS_CONV_K3S2 || c.kind == BTS_CONV_K3S2T)) return BTS_ERR_UNSUPPORTED;
  r = plan_wgrad(ch, ro.ntaps, ro.s, ro.neg, c.N, ro.Dp, ro.Hp, ro.Wp, ro.Cp, ro.Dq, ro.Hq, ro.Wq, ro.Cq);
  if (r != BTS_OK) return r;
  WgradParams& p = ch.p;
  const bool pIsDy = ro.transposed || ro.swapped;
  p.p = p.q = p.zeros = nullptr; p.partial = nullptr; p.partial_b = nullptr;      // (the launch's to fill in)
  p.ldp = pIsDy ? c.lddy : c.ldx;
  p.ldq = pIsDy ? c.ldx : c.lddy;
  // bias gradient = column sums of dy: dy is Q in the plain form only (the swapped form's comes from bts_colsum, the transposed has none)
  p.want_bias = (c.want_db && !pIsDy) ? 1 : 0;
  ch.ws_partial = 0;      // [nsp][npct][nqct][ntiles][32][32] floats, then [nsp][nqct][32] doubles
  ch.ws_partial_b = (long)ch.nsp * ch.npct * ch.nqct * p.ntiles * 1024 * 4;
  ch.ws_colsum = (ch.ws_partial_b + (long)ch.nsp * ch.nqct * 32 * 8 + 256 + 15) & ~15L;
  ch.colsum_bytes = ro.swapped ? bts_colsum_workspace(c.N, (long)c.D * c.H * c.W, c.Cout) : 0;
  ch.ws = ch.ws_colsum + ch.colsum_bytes + 128;
  ch.ws_zeros = (ch.ws - 64) & ~15L;
  // both operands 16-byte granular (leading dimensions, channel counts, base addresses)?  Without that, register staging; the fast
  // staging (p.fastf / p.fixg) also goes where its 32-bit offsets would not reach.
  const bool vec = (p.ldp % 4 == 0) && (p.Cp % 4 == 0) && (p.ldq % 4 == 0) && (p.Cq % 4 == 0) && c.x16 && c.dy16;
  if (p.fastf && ((double)p.IZ * p.Hp * p.Wp * p.ldp * 4.0 >= 4.0e9 || (double)p.TZ * p.Hq * p.Wq * p.ldq * 4.0 >= 4.0e9 || !vec))
    p.fastf = p.fixg = 0;
  ch.variant = !vec ? 0 : (p.fastf ? 1 + p.fixg : 1);
  static const int ksym[4] = {100, 104, 109, 110};
  ch.sym = ksym[ch.variant];
  ch.NV = (long)c.N * ro.Dq * ro.Hq * ro.Wq;
  ch.flops = 2.0 * ro.ntaps * (double)ro.Cp * ro.Cq * (double)ch.NV;
  // 1x1x1 convs on big grids, plain form: the streaming kernel (BTS_K1W=0: the staged kernel).  Stride-1 3x3x3 layers of whole
  // sub-tiles and 32-channel groups whose tile offsets fit 31 bits: Winograd form, all three axes (BTS_WGW=0: the direct fixed sweep).
  if (ro.ntaps == 1 && !pIsDy && p.ntiles == 1 && ch.NV >= 32768) {
    if (wg_switch_on("BTS_K1W")) ch.sym = 26;
  } else if (ch.variant == 2 && ro.ntaps == 27 && ro.s == 1 && wg_switch_on("BTS_WGW") &&
             5.0 * p.Hp * p.Wp * p.ldp * 4.0 < 2.0e9 && 3.0 * p.Hq * p.Wq * p.ldq * 4.0 < 2.0e9) {
    ch.sym = 24;
  }
  ch.clear_zeros = ch.sym == 104;
  return BTS_OK;
}

static WgCall wgrad_query_call(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned) {
  return WgCall{kind, N, D, H, W, Cin, ldx, Cout, lddy, 0, 0, aligned & 1, (aligned >> 1) & 1};
}

// workspace bytes for bts_conv3d_bwd_weight; (D,H,W) are the forward INPUT dims, Cin the slab (folded) count.  The shape alone decides.
extern "C" long bts_conv3d_bwd_weight_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  WgChoice ch;
  return wgrad_choose(wgrad_query_call(kind, N, D, H, W, Cin, Cin, Cout, Cout, 3), ch) == BTS_OK ? ch.ws : -1;
}

// Host only: the profile symbol of the kernel bts_conv3d_bwd_weight runs for the described call -- 100 | 104 | 109 | 110 wgrad_kernel
// (register staging | LDS-DMA staging | the fixed-geometry sweeps of stride 1 | 2), 24 wgw_kernel, 26 k1w_kernel -- or the negative
// status of a call it does not take.  aligned: bit 0 x, bit 1 dy on a 16-byte boundary.
extern "C" int bts_conv3d_bwd_weight_kernel(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned) {
  WgChoice ch;
  const int r = wgrad_choose(wgrad_query_call(kind, N, D, H, W, Cin, ldx, Cout, lddy, aligned), ch);
  return r != BTS_OK ? r : ch.sym;
}

// Host only: the form of that kernel -- 3 Winograd F(2x2x2,3x3x3) (wgw_kernel) | 0 every other -- or the negative status.
extern "C" int bts_conv3d_bwd_weight_form(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned) {
  const int k = bts_conv3d_bwd_weight_kernel(kind, N, D, H, W, Cin, ldx, Cout, lddy, aligned);
  return k < 0 ? k : (k == 24 ? 3 : 0);
}

// p: ch.p with the call's pointers
static int wgrad_launch(const WgChoice& ch, const WgradParams& p, hipStream_t stream) {
  typedef void (*WgKernel)(const WgradParams);
  static const WgKernel kernels[4] = {wgrad_kernel<0, 0>, wgrad_kernel<1, 0>, wgrad_kernel<2, 1>, wgrad_kernel<2, 2>};
  static bool attr_done = false;
  if (!attr_done) {
    for (int i = 0; i < 4; ++i) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[i]), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) return (int)e;
    }
    attr_done = true;
  }
  if (ch.clear_zeros) {
    hipError_t e = hipMemsetAsync(const_cast<float*>(p.zeros), 0, 64, stream);
    if (e != hipSuccess) return (int)e;
  }
  static bool wattr = false;
  if (ch.sym == 24 && !wattr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wgw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    wattr = true;
  }
  const dim3 grid(ch.nsp, ch.npct, ch.nqct);
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(ch.sym, ch.flops, stream);
  (void)hipGetLastError();
  switch (ch.sym) {
    case 26:
      hipLaunchKernelGGL(k1w_kernel, grid, dim3(K1W_THREADS), 0, stream, p, ch.NV, (((ch.NV + ch.nsp - 1) / ch.nsp) + 15) & ~15L);
      break;
    case 24:
      hipLaunchKernelGGL(wgw_kernel, grid, dim3(WGW_THREADS), (size_t)2 * WGW_BUF * sizeof(float), stream, p);
      break;
    default:
      hipLaunchKernelGGL(kernels[ch.variant], grid, dim3(WG_THREADS), ch.shmem, stream, p);
  }
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// dw is in the reference layout with Cin_ref = Cin + dup_shift input channels; db may be null.
extern "C" int bts_conv3d_bwd_weight(int kind, const float* x, const float* dy, float* dw, float* db, void* workspace,
                                     long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout,
                                     int lddy, int dup_start, int dup_shift, int accumulate, hipStream_t stream) {
  const WgCall c{kind, N, D, H, W, Cin, ldx, Cout, lddy, dup_shift, db != nullptr, (((uintptr_t)x) & 15) == 0, (((uintptr_t)dy) & 15) == 0};
  WgChoice ch;
  int r = wgrad_choose(c, ch);
  if (r != BTS_OK) return r;
  if (workspace_bytes < ch.ws || workspace == nullptr) return BTS_ERR_WORKSPACE;
  const WgradRoles& ro = ch.ro;
  const bool pIsDy = ro.transposed || ro.swapped;
  char* ws = reinterpret_cast<char*>(workspace);
  WgradParams p = ch.p;
  p.p = pIsDy ? dy : x;
  p.q = pIsDy ? x : dy;
  p.partial = reinterpret_cast<float*>(ws + ch.ws_partial);
  p.partial_b = reinterpret_cast<double*>(((uintptr_t)(ws + ch.ws_partial_b) + 15) & ~(uintptr_t)15);      // (a workspace off its boundary)
  p.zeros = reinterpret_cast<const float*>(ws + ch.ws_zeros);
  r = wgrad_launch(ch, p, stream);
  if (r != BTS_OK) return r;
  WfinParams f;
  f.partial = p.partial; f.partial_b = p.partial_b; f.dw = dw; f.db = p.want_bias ? db : nullptr;
  f.nsp = ch.nsp; f.npct = ch.npct; f.nqct = ch.nqct; f.ntaps = ro.ntaps; f.ntiles = p.ntiles; f.cpad = p.cpad;
  f.Cp = ro.Cp; f.Cq = ro.Cq;
  const int Cin_ref = Cin + dup_shift;
  f.sT = (long)Cin_ref * Cout;
  if (ro.transposed) { f.sP = Cin_ref; f.sQ = 1; f.fold_axis = 0; }   // (t, Cout, Cin): P = cout, Q = cin
  else if (ro.swapped) { f.sP = 1; f.sQ = Cout; f.fold_axis = 2; }     // (t, Cin, Cout): P = cout, Q = cin
  else { f.sP = Cout; f.sQ = 1; f.fold_axis = 1; }                     // (t, Cin, Cout): P = cin, Q = cout
  f.shift = dup_shift;
  f.dup_start = dup_shift > 0 ? dup_start : (1 << 30);
  f.accum = accumulate;
  long rows = (long)ro.ntaps * ro.Cp * ch.nqct;
  if (ch.nsp <= 16) {
    long blocks = (rows * 32 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    (void)hipGetLastError(); hipLaunchKernelGGL(wgrad_finalize_flat_kernel, dim3((int)blocks), dim3(256), 0, stream, f);
  } else {
    int blocks = (int)(rows < 4096 ? rows : 4096);
    (void)hipGetLastError(); hipLaunchKernelGGL(wgrad_finalize_kernel, dim3(blocks), dim3(256), 0, stream, f);
  }
  BTS_LAUNCH_CHECK();
  if (db != nullptr && ro.swapped)      // bias gradient of the swapped form: plain column sum of dy
    return bts_colsum(dy, db, ws + ch.ws_colsum, ch.colsum_bytes, N, (long)D * H * W, Cout, lddy, 1.0f, 1, accumulate, stream);
  return BTS_OK;
}
