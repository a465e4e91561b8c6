// The fp32 forward / data-gradient conv engine: no kernels here.  conv_choose offers a call to the kernels (conv_dsc.hip, conv_c2.hip,
// conv_wino3.hip, conv_wino.hip, conv_k1s.hip, conv_upm.hip, conv_igemm.hip) under the accept / launch contract of conv_plan.h; the
// extern "C" bts_conv3d_* entry points and host-only queries answer from it.  Fused forms: shortcut pair (second output), GroupNorm
// statistics in the epilogue, data-gradient pair (second input).
#include <stdlib.h>
#include "common.h"
#include "conv_plan.h"

// The kernel of a call, in the order the forms were always offered: 3x3x3 stride 1 -- the direct kernel (no second weight set), the
// two-channel kernel (Cin == 2, no second input), the Winograd forms (never with the sigmoid; the second form then runs as a 1x1x1 launch
// of its own: ch.second -- except the second INPUT of a large unsplit w3 launch, which w3_accept takes into the launch); 1x1x1 -- the
// streaming kernel; transposed -- the merged-class kernel (both without a second form); then the tiled kernel, whose status is that of a
// call no kernel takes.
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

// Ensures the image part the chosen kernel reads (3x3x3 stride 1: the Winograd forms their own, every other kernel the implicit-GEMM
// part), launches, and records the part as in use once the launch was accepted.
static int conv_launch(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
  const unsigned bit = c.geo != GEO_S1 ? 0u : ch.kernel == CONV_W3 ? IMG_W3 : ch.kernel == CONV_WINO ? IMG_WINO : IMG_IGEMM;
  if (bit) { const int e = bts_img_ensure_(q.wp, bit, stream); if (e != BTS_OK) return e; }
  int r;
  switch (ch.kernel) {
    case CONV_DSC: r = bts_dsc_launch_(c, ch, q, stream); break;
    case CONV_C2: r = bts_c2_launch_(c, ch, q, stream); break;
    case CONV_W3: r = bts_w3_launch_(c, ch, q, stream); break;
    case CONV_WINO: r = bts_wino_launch_(c, ch, q, stream); break;
    case CONV_K1S: r = bts_k1s_launch_(c, ch, q, stream); break;
    case CONV_UPM: r = bts_upm_launch_(c, ch, q, stream); break;
    default: r = bts_igemm_launch_(c, ch, q, stream); break;
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

// positive extents and channels, rows that hold them: the first thing every entry point asks
static bool conv_dims_ok(int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy) {
  return N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ldx >= Cin && ldy >= Cout;
}
// The call of a forward (dir 0) or data-gradient (dir 1) entry point; kind, (N, D, H, W, Cin, Cout) and the flags as the ABI names them,
// ldx / ldy: rows of the forward input / output (dir 1: of dx, the tensor written / of dy, the tensor read).  The data gradient of the
// stride-2 conv is the gather form over the fine grid's parity classes, that of the transposed conv the stride-2 'same' conv of dy.
static int conv_call_of(int dir, int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, int flags, ConvCall& c) {
  if (!conv_dims_ok(N, D, H, W, Cin, ldx, Cout, ldy)) return BTS_ERR_SHAPE;
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
// the operands a host-only query describes (bts_hip.h): `aligned` bit 0 x, 1 y, 2 the second operand, 3 the workspace on a 16-byte
// boundary; workspace_bytes < 0: as large as needed
static void conv_operand_view(ConvCall& c, int aligned, long workspace_bytes) {
  c.x16 = aligned & 1; c.y16 = (aligned >> 1) & 1; c.p2_16 = (aligned >> 2) & 1; c.ws16 = (aligned >> 3) & 1;
  c.ws_bytes = workspace_bytes < 0 ? LONG_MAX : workspace_bytes;
}
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
static long gnfuse_partial_bytes(int N, int Do, int Ho, int Wo, int Cout) {
  // upper bound of N*G*B*2 doubles: one pair per 64-voxel tile and 32-cout tile
  const long tiles = (long)N * ((Do + 0) ) * ((Ho + 3) / 4) * ((Wo + 7) / 8);
  return tiles * ((conv_npad32(Cout) + 31) / 32) * 2 * (long)sizeof(double) + 64;
}
extern "C" long bts_conv3d_fwd_gn_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout, int G) {
  const long cw = bts_conv3d_fwd_workspace(kind, N, D, H, W, Cin, Cout);
  ConvCall c;
  if (cw < 0 || conv_call_of(0, kind, N, D, H, W, Cin, Cin, Cout, Cout, 0, c) != BTS_OK) return -1;
  const long gw = bts_gn_workspace(N, (long)c.Do * c.Ho * c.Wo, Cout, G, BTS_GN_SLAB);
  if (gw < 0) return -1;
  const long fused = ((cw + 63) & ~63L) + gnfuse_partial_bytes(N, c.Do, c.Ho, c.Wo, Cout);
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
  if (!conv_dims_ok(N, D, H, W, Cin, ldx, Cout, Cout)) return BTS_ERR_SHAPE;      // (y is dense)
  if (((uintptr_t)workspace) & 15) return BTS_ERR_ALIGN;     // (the GroupNorm partials in it are read as double2: refuse before y is written)
  return conv_fwd_gn_impl(kind, x, wp_fwd, bias, y, nullptr, nullptr, nullptr, 0, workspace, workspace_bytes, N, D, H, W, Cin, ldx,
                          Cout, G, eps, mean, rstd, stream);
}
extern "C" int bts_conv3d_fwd_fused2_gn(const float* x, const float* wp_fwd, const float* bias, float* y, const float* wp2,
                                        const float* bias2, float* y2, void* workspace, long workspace_bytes, int N, int D, int H,
                                        int W, int Cin, int ldx, int Cout, int ldy2, int G, float eps, float* mean, float* rstd,
                                        hipStream_t stream) {
  if (!conv_dims_ok(N, D, H, W, Cin, ldx, Cout, ldy2) || !wp2 || !y2) return BTS_ERR_SHAPE;      // (y is dense, y2 has rows of ldy2)
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
  conv_operand_view(c, aligned, workspace_bytes);      // (fused: dy2 is aligned, pair_call_of asked for it)
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

// Which igemm_kernel<...> instantiation the tiled kernel would run a call on: cfg + SYM_IGEMM_K1 * (KGS==4); cfg ids: IgemmPlan (conv_plan.h).
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
// The profile symbol of the kernel that takes a call first (host only): SYM_UPM | K1S | DSC | C2 | WINO | W3 (conv_plan.h) | the tiled
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
  conv_operand_view(c, aligned, workspace_bytes);
  r = conv_choose(c, ch);
  return r != BTS_OK ? r : ch.sym;
}
