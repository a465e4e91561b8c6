// The fp32 weight gradient's engine: the roles of the operands, the tiling and K-split plan, the ONE choice per call (wgrad_plan.h), the
// queries that answer from it and the entry point.  The reference obtains these gradients from TF autodiff (train.py:142-151); the math
// is SURVEY Appendix A':
//   dW[t][pc][qc] = sum_{n,v} P[n, v*s + off_t, pc] * Q[n, v, qc]        db[qc] = sum_{n,v} Q[n, v, qc]
//     Conv3D k1 / k3s1 / k3s2 : P = layer input x, Q = dy  -> dW in (t, Cin, Cout)
//     Conv3DTranspose k3s2    : P = dy (fine grid, s=2), Q = x (coarse grid) -> dW in (t, Cout, Cin)
//     "swapped" k3s1          : P = dy, Q = x with negated tap offsets (u = v + off_t): used when Cout <= 8 so the
//                               tiny channel count sits on the packable P side
// Per-workgroup partials go to a workspace and are combined in a fixed order by the finalize pass (conv_wgfin.hip).
#include "wgrad_plan.h"

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
  p.lgSP = ilog2(SP);
  p.ntiles = (cpad == 32) ? ntaps : (ntaps * cpad + 31) / 32;
  // sub-tile: 128 voxels for s=1 (16x4x2), 32 voxels for s=2 (8x4x1); 1x1x1: 256 voxels (32x4x2)
  int TX, TY, TZ;
  if (ntaps == 1) { TX = 32; TY = 4; TZ = 2; }
  else if (s == 1) { TX = 16; TY = 4; TZ = 2; }
  else { TX = 8; TY = 4; TZ = 1; }
  while (TX > 2 && TX / 2 >= Wq) { TX /= 2; if (TY * 2 <= 8) TY *= 2; else TZ *= 2; }
  while (TY > 1 && TY / 2 >= Hq) { TY /= 2; TZ *= 2; }
  while (TZ > 1 && TZ / 2 >= Dq && TX * TY * (TZ / 2) >= 2) TZ /= 2;
  p.lgTX = ilog2(TX); p.lgTY = ilog2(TY); p.TZ = TZ;
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

static int wgrad_roles(WgradRoles& r, int kind, int D, int H, int W, int Cin, int Cout) {
  r.ntaps = (kind == BTS_CONV_K1) ? 1 : 27;
  r.s = 1; r.neg = 0; r.swapped = 0; r.transposed = 0; r.p_is_dy = 0;
  r.Dp = D; r.Hp = H; r.Wp = W; r.Cp = Cin; r.Dq = D; r.Hq = H; r.Wq = W; r.Cq = Cout;
  if (kind == BTS_CONV_K3S2) {
    if ((D | H | W) & 1) return BTS_ERR_SHAPE;
    r.s = 2; r.Dq = D / 2; r.Hq = H / 2; r.Wq = W / 2;
  } else if (kind == BTS_CONV_K3S2T) {  // P = dy on the fine grid (2D), Q = x on the coarse grid
    r.transposed = r.p_is_dy = 1;
    r.s = 2; r.Dp = 2 * D; r.Hp = 2 * H; r.Wp = 2 * W; r.Cp = Cout; r.Cq = Cin;
  } else if (kind == BTS_CONV_K3S1 && Cout <= 8 && Cin > Cout) {
    r.swapped = r.p_is_dy = 1; r.neg = 1; r.Cp = Cout; r.Cq = Cin;  // P = dy (tiny), Q = x
  }
  return BTS_OK;
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
  p.p = p.q = p.zeros = nullptr; p.partial = nullptr; p.partial_b = nullptr;      // (the launch's to fill in)
  p.ldp = ro.p_is_dy ? c.lddy : c.ldx;
  p.ldq = ro.p_is_dy ? c.ldx : c.lddy;
  // bias gradient = column sums of dy: dy is Q in the plain form only (the swapped form's comes from bts_colsum, the transposed has none)
  p.want_bias = (c.want_db && !ro.p_is_dy) ? 1 : 0;
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
  static const int mode_fixg[4] = {0 << 2 | 0, 1 << 2 | 0, 2 << 2 | 1, 2 << 2 | 2};      // wgrad_kernel<MODE, FIXG> of the variant
  ch.sym = SYM_WGRAD + mode_fixg[ch.variant];
  ch.NV = (long)c.N * ro.Dq * ro.Hq * ro.Wq;
  ch.flops = 2.0 * ro.ntaps * (double)ro.Cp * ro.Cq * (double)ch.NV;
  // 1x1x1 convs on big grids, plain form: the streaming kernel (BTS_K1W=0: the staged kernel).  Stride-1 3x3x3 layers of whole
  // sub-tiles and 32-channel groups whose tile offsets fit 31 bits: Winograd form, all three axes (BTS_WGW=0: the direct fixed sweep).
  if (ro.ntaps == 1 && !ro.p_is_dy && p.ntiles == 1 && ch.NV >= 32768) {
    if (conv_env_long("BTS_K1W", 1) != 0) ch.sym = SYM_K1W;
  } else if (ch.variant == 2 && ro.ntaps == 27 && ro.s == 1 && conv_env_long("BTS_WGW", 1) != 0 &&
             5.0 * p.Hp * p.Wp * p.ldp * 4.0 < 2.0e9 && 3.0 * p.Hq * p.Wq * p.ldq * 4.0 < 2.0e9) {
    ch.sym = SYM_WGW;
  }
  ch.clear_zeros = ch.sym == SYM_WGRAD + (1 << 2 | 0);
  return BTS_OK;
}

static WgCall wgrad_query_call(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned) {
  return WgCall{kind, N, D, H, W, Cin, ldx, Cout, lddy, 0, 0, 0, 0, aligned & 1, (aligned >> 1) & 1};
}

// workspace bytes for bts_conv3d_bwd_weight; (D,H,W) are the forward INPUT dims, Cin the slab (folded) count.  The shape alone decides.
extern "C" long bts_conv3d_bwd_weight_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout) {
  WgChoice ch;
  return wgrad_choose(wgrad_query_call(kind, N, D, H, W, Cin, Cin, Cout, Cout, 3), ch) == BTS_OK ? ch.ws : -1;
}

// Host only: the profile symbol of the kernel bts_conv3d_bwd_weight runs for the described call -- SYM_WGRAD + 0 | 4 | 9 | 10 wgrad_kernel
// (register staging | LDS-DMA staging | the fixed-geometry sweeps of stride 1 | 2), SYM_WGW wgw_kernel, SYM_K1W k1w_kernel -- or the
// negative status of a call it does not take.  aligned: bit 0 x, bit 1 dy on a 16-byte boundary.
extern "C" int bts_conv3d_bwd_weight_kernel(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned) {
  WgChoice ch;
  const int r = wgrad_choose(wgrad_query_call(kind, N, D, H, W, Cin, ldx, Cout, lddy, aligned), ch);
  return r != BTS_OK ? r : ch.sym;
}

// Host only: the form of that kernel -- 3 Winograd F(2x2x2,3x3x3) (wgw_kernel) | 0 every other -- or the negative status.
extern "C" int bts_conv3d_bwd_weight_form(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned) {
  const int k = bts_conv3d_bwd_weight_kernel(kind, N, D, H, W, Cin, ldx, Cout, lddy, aligned);
  return k < 0 ? k : (k == SYM_WGW ? 3 : 0);
}

// dw is in the reference layout with Cin_ref = Cin + dup_shift input channels; db may be null.
extern "C" int bts_conv3d_bwd_weight(int kind, const float* x, const float* dy, float* dw, float* db, void* workspace,
                                     long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout,
                                     int lddy, int dup_start, int dup_shift, int accumulate, hipStream_t stream) {
  const WgCall c{kind, N, D, H, W, Cin, ldx, Cout, lddy, dup_start, dup_shift, db != nullptr, accumulate,
                 (((uintptr_t)x) & 15) == 0, (((uintptr_t)dy) & 15) == 0};
  WgChoice ch;
  int r = wgrad_choose(c, ch);
  if (r != BTS_OK) return r;
  if (workspace_bytes < ch.ws || workspace == nullptr) return BTS_ERR_WORKSPACE;
  const WgradRoles& ro = ch.ro;
  char* ws = reinterpret_cast<char*>(workspace);
  WgradParams p = ch.p;
  p.p = ro.p_is_dy ? dy : x;
  p.q = ro.p_is_dy ? x : dy;
  p.partial = reinterpret_cast<float*>(ws + ch.ws_partial);
  p.partial_b = reinterpret_cast<double*>(((uintptr_t)(ws + ch.ws_partial_b) + 15) & ~(uintptr_t)15);      // (a workspace off its boundary)
  p.zeros = reinterpret_cast<const float*>(ws + ch.ws_zeros);
  switch (ch.sym) {
    case SYM_K1W: r = bts_k1w_launch_(ch, p, stream); break;
    case SYM_WGW: r = bts_wgw_launch_(ch, p, stream); break;
    default: r = bts_wgrad_direct_launch_(ch, p, stream);
  }
  if (r != BTS_OK) return r;
  r = bts_wgrad_finalize_(c, ch, p, dw, db, stream);
  if (r != BTS_OK) return r;
  if (db != nullptr && ro.swapped)      // bias gradient of the swapped form: plain column sum of dy
    return bts_colsum(dy, db, ws + ch.ws_colsum, ch.colsum_bytes, N, (long)D * H * W, Cout, lddy, 1.0f, 1, accumulate, stream);
  return BTS_OK;
}
