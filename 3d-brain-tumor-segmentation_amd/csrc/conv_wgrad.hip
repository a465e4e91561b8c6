// The direct kernel of the weight (and bias) gradients of the 3-D convolutions on the exact-fp32 matrix pipe:
//   dW[t][pc][qc] = sum_{n,v} P[n, v*s + off_t, pc] * Q[n, v, qc]        db[qc] = sum_{n,v} Q[n, v, qc]
// (which of x, dy is P and which Q, per form: conv_wgrad_engine.hip).
// GEMM view: M = 32 rows (P channels of one tap, or -- when P has <= 16 channels -- packed (tap, channel) pairs),
// N = 32 Q-channels, K = voxels (v_mfma_f32_32x32x2_f32 consumes 2 voxels per instruction).
// A 512-thread workgroup (8 waves) walks a run of spatial sub-tiles; the waves split the row-tiles (27 taps) or, when
// there are at most 4 row-tiles, the voxel pairs.  P halo tile and Q tile live in LDS as [voxel][channels] so both
// fragment reads are conflict-free ds_read_b32; the next sub-tile is staged by direct global->LDS DMA
// (global_load_lds_dwordx4) while the current one is multiplied (double-buffered LDS, one barrier per sub-tile).
// Kernel variants <MODE, FIXG>: <2,1>/<2,2> straight-line fixed-geometry sweeps with interleaved staging for every big
// 3x3x3 layer (stride 1 / 2), <1,0> general LDS-DMA staging, <0,0> register staging for odd strides / channel counts.
// Per-workgroup partials go to a workspace and are combined in a fixed order by the finalize pass (conv_wgfin.hip).
#include <type_traits>
#include "wgrad_plan.h"

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

  // One sub-tile: its place in the tile grid, the origins of its Q tile (o) and of its P halo tile (i), and the operands there.
  // The origins are wave-uniform and may be negative for the halo: pointer arithmetic stays scalar.
  struct WgSub {
    int tz, ty, tx, oz0, oy0, ox0, iz0, iy0, ix0;
    const float *pbase, *qbase;
  };
  auto decode = [&](int sub) {
    WgSub t;
    int b = sub;
    t.tx = b % p.ntx; b /= p.ntx;
    t.ty = b % p.nty; b /= p.nty;
    t.tz = b % p.ntz;
    const int n = b / p.ntz;
    t.oz0 = t.tz * p.TZ; t.oy0 = t.ty * TY; t.ox0 = t.tx * TX;
    t.iz0 = t.oz0 * p.s + p.loz; t.iy0 = t.oy0 * p.s + p.loy; t.ix0 = t.ox0 * p.s + p.lox;
    t.pbase = p.p + ((((long)n * p.Dp + t.iz0) * p.Hp + t.iy0) * p.Wp + t.ix0) * (long)p.ldp;
    t.qbase = p.q + ((((long)n * p.Dq + t.oz0) * p.Hq + t.oy0) * p.Wq + t.ox0) * (long)p.ldq;
    return t;
  };
  // One staging slot: the voxel inside the tile and the first channel of its quad; is it inside the image and the channels; its
  // offset from the tile's origin (elements).  P: the halo tile, [voxel][SP]; Q: [m][32].
  struct WgSlot { int z, y, x, c; };
  auto slot_p = [&](int e) {
    WgSlot v;
    const int vox = e >> (p.lgSP - 2), qd = e & (qpvP - 1);
    v.z = fast_div(vox, invIYX);
    const int r = vox - v.z * IYX;
    v.y = fast_div(r, invIX);
    v.x = r - v.y * p.IX;
    v.c = pc0 + qd * 4;
    return v;
  };
  auto in_p = [&](const WgSub& t, const WgSlot& v) {
    return (unsigned)(t.iz0 + v.z) < (unsigned)p.Dp && (unsigned)(t.iy0 + v.y) < (unsigned)p.Hp &&
           (unsigned)(t.ix0 + v.x) < (unsigned)p.Wp && v.c < p.Cp;
  };
  auto rel_p = [&](const WgSlot& v) { return ((v.z * p.Hp + v.y) * p.Wp + v.x) * p.ldp + v.c; };
  auto slot_q = [&](int e) {
    WgSlot v;
    const int m = e >> 3, qd = e & 7;
    v.z = m >> (p.lgTX + p.lgTY); v.y = (m >> p.lgTX) & (TY - 1); v.x = m & (TX - 1);
    v.c = qct * 32 + qd * 4;
    return v;
  };
  auto in_q = [&](const WgSub& t, const WgSlot& v) {
    return t.oz0 + v.z < p.Dq && t.oy0 + v.y < p.Hq && t.ox0 + v.x < p.Wq && v.c < p.Cq;
  };
  auto rel_q = [&](const WgSlot& v) { return ((v.z * p.Hq + v.y) * p.Wq + v.x) * p.ldq + v.c; };

  f32x4 preP[WG_PSLOTS], preQ[WG_QSLOTS];
  auto fetch = [&](int sub) {
    const WgSub t = decode(sub);
#pragma unroll
    for (int i = 0; i < WG_PSLOTS; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      const int e = tid + i * WG_THREADS;
      if (e < nPslots) {
        const WgSlot sl = slot_p(e);
        if (in_p(t, sl)) {
          const float* src = t.pbase + rel_p(sl);
          if (vecP) v = *reinterpret_cast<const f32x4*>(src);
          else {
            v[0] = src[0];
            if (sl.c + 1 < p.Cp) v[1] = src[1];
            if (sl.c + 2 < p.Cp) v[2] = src[2];
            if (sl.c + 3 < p.Cp) v[3] = src[3];
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
        const WgSlot sl = slot_q(e);
        if (in_q(t, sl)) {
          const float* src = t.qbase + rel_q(sl);
          if (vecQ) v = *reinterpret_cast<const f32x4*>(src);
          else {
            v[0] = src[0];
            if (sl.c + 1 < p.Cq) v[1] = src[1];
            if (sl.c + 2 < p.Cq) v[2] = src[2];
            if (sl.c + 3 < p.Cq) v[3] = src[3];
          }
        }
      }
      preQ[i] = v;
    }
  };
  // direct-to-LDS staging of one sub-tile into buffer `buf` (every lane of every issuing wave is active)
  auto fetch_glds = [&](int sub, float* buf) {
    const WgSub t = decode(sub);
#pragma unroll
    for (int i = 0; i < WG_PSLOTS; ++i) {
      const int e0 = wave * 64 + i * WG_THREADS;  // wave-uniform first slot of this wave-load
      if (e0 * 4 < pRegion) {
        const int e = e0 + lane;
        const float* src = p.zeros;
        if (e < nPslots) {
          const WgSlot sl = slot_p(e);
          if (in_p(t, sl)) src = t.pbase + rel_p(sl);
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
          const WgSlot sl = slot_q(e);
          if (in_q(t, sl)) src = t.qbase + rel_q(sl);
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
  // (The table below spells slot_p / rel_p and slot_q / rel_q out once more, for 32-channel voxels and without the bounds: filled
  // through them, the two fixed-sweep kernels compile to other code.)
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
    const WgSub t = decode(sub);
    f_pbase = reinterpret_cast<const char*>(t.pbase);
    f_qbase = reinterpret_cast<const char*>(t.qbase);
    // faces of the halo tile that lie outside the image (stride 1: one-voxel halo on both sides; stride 2: high side only)
    const unsigned lowf = p.loz < 0 ? 1u : 0u;
    f_tmask = ((t.tz == 0) ? lowf : 0u) | ((t.tz == p.ntz - 1) ? 2u : 0u) | ((t.ty == 0) ? 4u * lowf : 0u) |
              ((t.ty == p.nty - 1) ? 8u : 0u) | ((t.tx == 0) ? 16u * lowf : 0u) | ((t.tx == p.ntx - 1) ? 32u : 0u);
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

  // ---- write partials ----  (the cross-wave sum is written out at both places, as it is in k1w_kernel: through one function or
  // lambda every variant compiles to other code)
  const long tileBase = wg_partial_base(pct, qct, p.ntiles);
  if constexpr (FIXG != 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // the wave's own tiles w, w+8, w+16
      float* dst = p.partial + tileBase + (long)(wave + WG_WAVES * i) * 1024;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[wg_acc_row(r, h) * 32 + l32] = acc[i][r];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // tiles 24..26: fixed-order sum of the 8 waves' K-slices through LDS
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) lds[wave * 1024 + wg_acc_row(r, h) * 32 + l32] = accx[i][r];
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
        for (int r = 0; r < 16; ++r) dst[wg_acc_row(r, h) * 32 + l32] = acc[i][r];
      }
    }
  } else {
    // cross-wave fixed-order reduction through LDS (staging buffers are free now)
#pragma unroll
    for (int i = 0; i < WG_MAXT; ++i) {
      if (i < p.ntiles) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) lds[wave * 1024 + wg_acc_row(r, h) * 32 + l32] = acc[i][r];
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
  if (p.want_bias && pct == 0) wg_bias_partial(lds, bsum, p, qct, tid);
}

// p: ch.p with the call's pointers
int bts_wgrad_direct_launch_(const WgChoice& ch, const WgradParams& p, hipStream_t stream) {
  typedef void (*WgKernel)(const WgradParams);
  static const WgKernel kernels[4] = {wgrad_kernel<0, 0>, wgrad_kernel<1, 0>, wgrad_kernel<2, 1>, wgrad_kernel<2, 2>};      // by ch.variant
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
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(ch.sym, ch.flops, stream);
  (void)hipGetLastError();
  hipLaunchKernelGGL(kernels[ch.variant], dim3(ch.nsp, ch.npct, ch.nqct), dim3(WG_THREADS), ch.shmem, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
