// The fp32 conv engine's host-side plan (conv_engine.hip; the kernels: conv_igemm.hip, conv_upm.hip, conv_k1s.hip, conv_dsc.hip, conv_c2.hip,
// conv_wino.hip, conv_wino3.hip): which kernel takes a call is decided ONCE per query or launch by conv_choose; queries and entry points
// answer from it, launchers neither decline nor re-plan.
#pragma once
#include <limits.h>
#include <stdlib.h>
#include "bts_internal.h"

#define IG_FLAG_BIAS 1
#define IG_FLAG_ACCUM 2
#define IG_FLAG_SIGMOID 4
#define IG_FLAG_VECIN 8
#define IG_FLAG_VECOUT 16

enum Geo { GEO_K1 = 0, GEO_S1 = 1, GEO_DOWN = 2, GEO_UP = 3 };      // UP: the 8 output-parity classes of the transposed form, one launch
enum { CONV_Y2 = 1, CONV_X2 = 2 };
struct ConvCall {         // geometry, shape, strides (elements), requested form and what the operands allow -- no pointers
  int geo;
  int N, Di, Hi, Wi;      // the tensor the taps read
  int Do, Ho, Wo;         // the tensor written: (Di, Hi, Wi) | half (DOWN) | twice (UP)
  int Cin, ldx, Cout, ldy;
  int flags;              // IG_FLAG_BIAS | ACCUM | SIGMOID
  int second;             // CONV_Y2: fused shortcut output y2 = 1x1x1 conv of x (rows of ld2) | CONV_X2: y += 1x1x1 conv of a second input x2 (rows of ld2)
  int ld2;
  int G;                  // GroupNorm partial sums of y, slab mode, G groups (0: none asked for)
  int x16, y16, p2_16, ws16;      // x / y / (y2 | x2) / the workspace on a 16-byte boundary
  long ws_bytes;          // workspace available (0: none) -- it changes the choice: the Winograd forms and the tiled kernel do not split without it, upm declines
};
// tile grid and k-split of a Winograd launch (xw: conv_wino.hip's tile width, 16 | 32); need: the bytes the shape's FULL split wants
struct WinoPlan { int xw, ntz, nty, ntx, nb, ksplit, kg_per, gn_zt; long wgs, need; };
typedef WinoPlan W3Plan;
struct UpmPlan { int lgTX, lgTY, TZ, ntz, nty, ntx, IZ, IY, IX, ksplit, kg_per; long need; };
// the tiled kernel: cfg ids 0:(2,1,4,1) M256 N32 | 1:(2,2,4,1) M256 N64 | 2:(1,2,2,2) M64 N128 | 3:(1,1,2,2) M64 N64 | 4:(1,1,4,1) M128 N32
struct IgemmPlan { int cfg, lgTX, lgTY, TZ, ntz, nty, ntx, IZ, IY, IX, gridy, ksplit, kg_per, gn_zt; long need; };
enum { CONV_DSC = 1, CONV_C2, CONV_W3, CONV_WINO, CONV_K1S, CONV_UPM, CONV_IGEMM };
// profile symbols (bts_prof_begin; names: ops.kernel_symbol); the tiled kernel's is its cfg + SYM_IGEMM_K1 * (1x1x1 staging), the direct
// weight-gradient kernel's (wgrad_plan.h) SYM_WGRAD + (MODE << 2 | FIXG) of wgrad_kernel<MODE, FIXG>
enum { SYM_IGEMM_K1 = 8, SYM_UPM = 20, SYM_K1S = 21, SYM_DSC = 22, SYM_WINO = 23, SYM_WGW = 24, SYM_C2 = 25, SYM_K1W = 26, SYM_W3 = 27,
       SYM_WGRAD = 100 };
struct ConvChoice {
  int kernel;             // CONV_DSC | C2 | W3 | WINO | K1S | UPM | IGEMM
  int sym;                // its profile symbol (SYM_*)
  union { WinoPlan w; UpmPlan u; IgemmPlan g; };      // the plan of `kernel` (dsc, c2, k1s: a grid that follows from the call)
  long ws;                // workspace bytes the launch uses (its split-K partials; 0: none)
  long gn_B;              // GroupNorm partial slots per (sample, group) it writes; 0: it cannot, or none asked for
  int second;             // c.second where the kernel leaves it to a 1x1x1 launch of its own (the Winograd forms; w3 takes CONV_X2 itself where w3_accept says so), else 0
};
// the operands of a launch (NULL: absent); wp = the whole image, wp2 = the K1 image of the second form, gnp = the partial slots
struct ConvPtrs { const float *x, *wp, *bias; float* y; const float *wp2, *bias2; float* y2; const float* x2; void* ws; double* gnp; };

inline int conv_npad32(int n) { return (n + 31) / 32 * 32; }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }      // of the next power of two
inline long conv_env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }      // (read per call: tests and A/B runs toggle them)
// z-tiles of TZ planes per GroupNorm slab group; 0: the groups do not hold whole tiles, or BTS_IGEMM_NOGNFUSE is set
inline int conv_gn_zt(const ConvCall& c, int TZ) {
  if (c.G <= 0 || c.Do % c.G != 0 || (c.Do / c.G) % TZ != 0 || getenv("BTS_IGEMM_NOGNFUSE") != nullptr) return 0;
  return (c.Do / c.G) / TZ;
}
// The k-split both Winograd forms give a tile grid of q.wgs workgroups that cannot fill the chip (fewer than `below`: split towards `target`,
// at least 4 k-groups per workgroup, at most 16 ways): q.ksplit, q.kg_per, q.need
inline void wino_split(WinoPlan& q, int N, int D, int H, int W, int Cin, long below, long target) {
  const int KG = Cin / 8;
  q.ksplit = 1;
  q.kg_per = KG;
  q.need = 0;
  if (q.wgs >= below || KG < 8) return;
  int ks = (int)((target + q.wgs - 1) / q.wgs);
  if (ks > KG / 4) ks = KG / 4;
  if (ks > 16) ks = 16;
  if (ks < 2) return;
  const int per = (KG + ks - 1) / ks;
  ks = (KG + per - 1) / per;
  if (ks < 2) return;
  q.ksplit = ks;
  q.kg_per = per;
  q.need = (long)ks * N * D * H * W * (q.nb * 32) * 4;
}
// What the two Winograd forms ask of a call before their own tile plan (the switches are each form's own) ...
inline bool wino_call_ok(const ConvCall& c) {
  if (c.ldx % 4 != 0 || c.ldy % 4 != 0 || !c.x16 || !c.y16) return false;
  return ((long)(c.Di + 2) * c.Hi * c.Wi + 64) * (long)c.ldx * 4 < 0x7fffffffL;      // 31-bit byte offsets inside one volume
}
// ... and after it: the output side's 31-bit bound, no split without a usable workspace, enough workgroups, the GroupNorm slots
inline bool wino_plan_ok(const ConvCall& c, ConvChoice& ch) {
  WinoPlan& q = ch.w;
  // voxel index * (ldy, or the padded split-K row) * 4, 0x80000000 = masked lane
  const long orow = (long)c.ldy > (long)q.nb * 32 ? (long)c.ldy : (long)q.nb * 32;
  if (((long)c.Di * c.Hi * c.Wi + 64) * orow * 4 >= 0x7fffffffL) return false;
  if (q.ksplit > 1 && (c.ws_bytes < q.need || !c.ws16)) { q.ksplit = 1; q.kg_per = c.Cin / 8; }
  if (q.wgs * q.ksplit < conv_env_long("BTS_WINO_MIN_WGS", 192)) return false;
  ch.ws = q.ksplit > 1 ? q.need : 0;
  q.gn_zt = q.ksplit == 1 ? conv_gn_zt(c, 4) : 0;
  ch.gn_B = (long)q.gn_zt * q.nty * q.ntx * q.nb;
  return true;
}

// true: the kernel takes the call (every switch, shape, stride, alignment, 31-bit and grid-size condition of its launcher) -- its plan,
// ws and gn_B are filled in, and the launcher does not decline it.  Which form goes to which kernel is conv_choose's rule.
bool w3_accept(const ConvCall& c, ConvChoice& ch);        // conv_wino3.hip: Winograd F(2x2x2,3x3x3), the third part of the K3S1 image
bool wino_accept(const ConvCall& c, ConvChoice& ch);      // conv_wino.hip: Winograd F(2x2,3x3) x direct, the second part
bool upm_accept(const ConvCall& c, ConvChoice& ch);       // conv_upm.hip: the merged-class transposed form
bool k1s_accept(const ConvCall& c, ConvChoice& ch);       // conv_k1s.hip: the streaming 1x1x1 conv
bool dsc_accept(const ConvCall& c, ConvChoice& ch);       // conv_dsc.hip: 3x3x3 into <= 4 output channels
bool c2_accept(const ConvCall& c, ConvChoice& ch);        // conv_c2.hip: 3x3x3 of a 2-channel input
int igemm_accept(const ConvCall& c, ConvChoice& ch);      // conv_igemm.hip: the tiled kernel takes every call of the family, so a status
// workspace the form's full split wants for a shape (0: none, or the form is switched off): the workspace queries size for every form
long w3_ws_need(const ConvCall& c);
long wino_ws_need(const ConvCall& c);
int bts_w3_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream);
int bts_wino_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream);
int bts_upm_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream);
int bts_k1s_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream);
int bts_dsc_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream);
int bts_c2_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream);
int bts_igemm_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream);
