// The fp32 weight gradient's host-side plan and the pieces its kernels share (conv_wgrad_engine.hip; the kernels: conv_wgrad.hip,
// conv_wgw.hip, conv_k1w.hip; the finalize pass: conv_wgfin.hip): which kernel takes a call, on which grid, and where its workspace areas
// lie is decided ONCE per query or launch by wgrad_choose; queries and the entry point answer from it, launchers neither decline nor
// re-plan.  Every kernel leaves per-workgroup partial tiles in the one layout the finalize pass combines in a fixed order.
#pragma once
#include "common.h"
#include "conv_plan.h"

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

// ---- ONE choice per call: which kernel takes it, on which grid, and where its workspace areas lie.  wgrad_choose makes it; the
// queries and the launch answer from it ----
struct WgCall {           // kind, shape, strides (elements), fold and what the operands allow -- no pointers
  int kind;
  int N, D, H, W;         // the forward INPUT dims
  int Cin, ldx, Cout, lddy;      // Cin: the slab (folded) count
  int dup_start, dup_shift;
  int want_db, accumulate;
  int x16, dy16;          // x / dy on a 16-byte boundary
};
struct WgradRoles {
  int ntaps, s, neg, swapped, transposed;
  int p_is_dy;            // P = dy, Q = x (the transposed and the swapped form); else P = x, Q = dy
  int Dp, Hp, Wp, Cp, Dq, Hq, Wq, Cq;
};
struct WgChoice {
  WgradRoles ro;
  WgradParams p;          // as planned, without its pointers
  int nsp, npct, nqct;
  size_t shmem;
  int variant;            // staging of wgrad_kernel: 0 register | 1 LDS-DMA | 2, 3 the fixed-geometry sweeps (stride 1, 2)
  int sym;                // profile symbol of the kernel that runs: SYM_WGRAD + (MODE << 2 | FIXG) of `variant` | SYM_WGW | SYM_K1W
  long NV;                // voxels of Q: the contraction length
  double flops;           // what the launch is profiled with
  int clear_zeros;        // the kernel reads the zero tail: the padding lanes of the general LDS-DMA staging only
  // workspace, byte offsets: partials | bias partials | column sums of dy (swapped form's db; colsum_bytes of them) | 64 zero bytes; ws: all
  long ws_partial, ws_partial_b, ws_colsum, colsum_bytes, ws_zeros, ws;
};

// p: ch.p with the call's pointers.  Each brackets its launch for the profiler with ch.sym and ch.flops.
int bts_wgrad_direct_launch_(const WgChoice& ch, const WgradParams& p, hipStream_t stream);      // conv_wgrad.hip: wgrad_kernel<MODE, FIXG> of ch.variant
int bts_wgw_launch_(const WgChoice& ch, const WgradParams& p, hipStream_t stream);               // conv_wgw.hip: Winograd F(2x2x2,3x3x3)
int bts_k1w_launch_(const WgChoice& ch, const WgradParams& p, hipStream_t stream);               // conv_k1w.hip: the streaming 1x1x1 kernel
// conv_wgfin.hip: dw (+)= the fixed-order sum of the partials, in the reference layout of the call's form; db (NULL: none) likewise
int bts_wgrad_finalize_(const WgCall& c, const WgChoice& ch, const WgradParams& p, float* dw, float* db, hipStream_t stream);

// ---- what the kernels share: their waves hold 32x32 tiles in v_mfma_f32_32x32x2_f32 accumulators.  A kernel uses a piece only where it
// compiles to the code the expression written out compiles to; where it does not, the kernel keeps the expression and says so. ----
template <int I>
struct IC { static constexpr int value = I; };      // a step or slot number handed to a lambda as a compile-time constant
// row of accumulator register r in the tile, for the lanes of half-wave h (the column is the lane's l32)
__device__ __forceinline__ int wg_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// first float of this workgroup's partial tiles, [blockIdx.x][pct][qct][ntiles][32][32]
__device__ __forceinline__ long wg_partial_base(int pct, int qct, int ntiles) {
  return ((((long)blockIdx.x * gridDim.y + pct) * gridDim.z + qct) * ntiles) * 1024;
}
// bias partial of a 512-thread workgroup: thread (c = tid & 31, part = tid >> 5) brings the column sum bsum of its 16th of Q's voxels
__device__ __forceinline__ void wg_bias_partial(float* lds, double bsum, const WgradParams& p, int qct, int tid) {
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
