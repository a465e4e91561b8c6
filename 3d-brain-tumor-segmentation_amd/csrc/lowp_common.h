// Storage-type traits, small helpers and the host-side kernel plans shared by the 16-bit translation units (lowp*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.h"
#include "bts_internal.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));

#define LP_F16 1
#define LP_BF16 2

// ---- storage-type traits: conversions are explicit, sums never happen in 16 bits ----
struct TF16 {
  typedef h16x8 frag;
  static __device__ __forceinline__ float ld(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ unsigned short st(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }   // RNE
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  }
};
struct TBF16 {
  typedef b16x8 frag;
  static __device__ __forceinline__ float ld(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }
  static __device__ __forceinline__ unsigned short st(float f) {   // round to nearest even: v_cvt_pk_bf16_f32 (NaN stays NaN)
    return __builtin_bit_cast(unsigned short, (__bf16)f);
  }
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b16x8, a), __builtin_bit_cast(b16x8, b), c, 0, 0, 0);
  }
};
// The trait type of a run-time dtype: f(TF16{}) for LP_F16, else f(TBF16{}) (entry points answer BTS_ERR_UNSUPPORTED for any other value
// before they get here).  f is a generic lambda -- `[&](auto t) { using T = decltype(t); ...<T>... }` -- so a typed launch is written once.
template <typename F> inline auto lp_typed(int dtype, F&& f) {
  if (dtype == LP_F16) return f(TF16{});
  return f(TBF16{});
}
template <typename T> __device__ __forceinline__ unsigned pack2(float a, float b) {
  return (unsigned)T::st(a) | ((unsigned)T::st(b) << 16);
}
typedef __bf16 b16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2_ __attribute__((ext_vector_type(2)));
template <> __device__ __forceinline__ unsigned pack2<TBF16>(float a, float b) {   // one v_cvt_pk_bf16_f32
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_{a, b}, b16x2));
}
template <typename T> __device__ __forceinline__ void unpack8(u32x4 v, float (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { o[2 * i] = T::ld((unsigned short)(v[i] & 0xffffu)); o[2 * i + 1] = T::ld((unsigned short)(v[i] >> 16)); }
}
template <typename T> __device__ __forceinline__ u32x4 pack8(const float (&o)[8]) {
  return u32x4{pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3]), pack2<T>(o[4], o[5]), pack2<T>(o[6], o[7])};
}
__device__ __forceinline__ u32x4 bload16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
}

// one register quad (4 consecutive couts) of a result: bias added by the caller; optional read-modify-write accumulation
template <typename T>
__device__ __forceinline__ void lp_store_quad(unsigned short* dst, float o0, float o1, float o2, float o3, int nleft, int accum) {
  if (nleft >= 4) {
    if (accum) {
      const u32x2 old = *reinterpret_cast<const u32x2*>(dst);
      o0 += T::ld((unsigned short)(old[0] & 0xffffu)); o1 += T::ld((unsigned short)(old[0] >> 16));
      o2 += T::ld((unsigned short)(old[1] & 0xffffu)); o3 += T::ld((unsigned short)(old[1] >> 16));
    }
    *reinterpret_cast<u32x2*>(dst) = u32x2{pack2<T>(o0, o1), pack2<T>(o2, o3)};
  } else {
    const float o[3] = {o0, o1, o2};
    for (int j = 0; j < nleft; ++j) dst[j] = T::st(accum ? o[j] + T::ld(dst[j]) : o[j]);
  }
}

// ---- weight packing: source addressing shared by every packed-image layout ----
struct LpPackParams {
  const float* w;
  unsigned short* wp;
  int ntaps, K, N, KS, NB;
  long sT, sK, sN;    // source strides of (tap, contraction index k, column n)
  int flip;           // tap t reads source tap ntaps-1-t (stride-1 data gradient)
  int cin_is_k;       // 1: the (possibly folded) input-channel axis is k (forward role), 0: it is n (data-gradient role)
  int shift, dup_start;
};
// source value of packed position (tap t, k, n) -- same conventions as the fp32 images (conv_pack.hip: pack_src)
__device__ __forceinline__ float lp_pack_src(const LpPackParams& q, int t, int k, int n) {
  if (k >= q.K || n >= q.N) return 0.f;
  const int ts = q.flip ? (q.ntaps - 1 - t) : t;
  int kk = k, nn = n, k2 = -1, n2 = -1;
  if (q.cin_is_k == 1) {
    // slab channel c is reference channel c + shift; inside [dup_start, ...) it is ALSO reference channel c - dup_start
    // (encoder.py:83-87: [o_{j-1}, o_0 .. o_{j-1}] read once from the slab [o_0 .. o_{j-1}])
    if (k >= q.dup_start) k2 = k - q.dup_start;
    kk = k + q.shift;
    n2 = n;
  } else {
    if (n >= q.dup_start) n2 = n - q.dup_start;
    nn = n + q.shift;
    k2 = k;
  }
  float v = q.w[ts * q.sT + kk * q.sK + nn * q.sN];
  if (q.shift > 0 && k2 >= 0 && n2 >= 0 && k2 < (q.cin_is_k ? q.shift : q.K) && n2 < (q.cin_is_k ? q.N : q.shift))
    v += q.w[ts * q.sT + k2 * q.sK + n2 * q.sN];
  return v;
}

// element i of the LDS-DMA stage-order part of a K3S1 image: [cout group of CBW blocks][k-step][dz][dy*3+dx][k-half][cout in group][8 cin]
// (lowp_s1d.hip's pack kernel and lowp_pack.hip's batched pack)
template <typename T> __device__ __forceinline__ void lp_s1d_pack_elem(const LpPackParams& p, int CBW, long i) {
  const int e = (int)(i & 7);
  long q = i >> 3;
  const int row = (int)(q % (32 * CBW)); q /= 32 * CBW;
  const int hh = (int)(q & 1); q >>= 1;
  const int t9 = (int)(q % 9); q /= 9;
  const int dz = (int)(q % 3); q /= 3;
  const int ks = (int)(q % p.KS);
  const int cg = (int)(q / p.KS);
  p.wp[i] = T::st(lp_pack_src(p, dz * 9 + t9, ks * 16 + hh * 8 + e, cg * CBW * 32 + row));
}


// 4 x 4 transpose of 16-byte pieces between the four lanes of a quad (lane bits 0-1) and four registers: afterwards register j of quad
// lane b holds what register b of quad lane j held.  Two butterfly stages of quad-permute DPP moves; its own inverse.
// What it is for: NDHWC rows of 64 channels are 128 bytes = 8 pieces.  The matrix instruction wants lane (voxel, k-half h) to hold piece
// 2 ks + h of ITS voxel in the register of k-step ks -- loaded that way, one instruction touches 32 bytes of each of 32 rows, four
// instructions per cache line, and the L1 request rate (not HBM) bounds the kernel at ~4 TB/s.  Loaded transposed -- instruction i:
// quad lane b fetches piece 2 b + h of voxel (quad base + i) -- an instruction covers 8 whole rows; the transpose then hands every lane
// its own voxel.  The same on the way out for 64-cout groups.
__device__ __forceinline__ void k1_quad_transpose(u32x4 (&r)[4], int b) {
  u32x4 s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u32x4 t;
#pragma unroll
    for (int d = 0; d < 4; ++d) t[d] = (unsigned)__builtin_amdgcn_mov_dpp((int)r[j ^ 1][d], 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    const bool keep = ((b ^ j) & 1) == 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) s[j][d] = keep ? r[j][d] : t[d];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u32x4 t;
#pragma unroll
    for (int d = 0; d < 4; ++d) t[d] = (unsigned)__builtin_amdgcn_mov_dpp((int)s[j ^ 2][d], 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    const bool keep = ((b ^ j) & 2) == 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) r[j][d] = keep ? s[j][d] : t[d];
  }
}

// the 2 x 2 form: register j of pair lane b <-> register b of pair lane j (64-byte row chunks: two k-steps)
__device__ __forceinline__ void k1_pair_transpose(u32x4 (&r)[2], int b) {
  u32x4 s[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    u32x4 t;
#pragma unroll
    for (int d = 0; d < 4; ++d) t[d] = (unsigned)__builtin_amdgcn_mov_dpp((int)r[j ^ 1][d], 0xB1, 0xf, 0xf, true);
    const bool keep = ((b ^ j) & 1) == 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) s[j][d] = keep ? r[j][d] : t[d];
  }
  r[0] = s[0]; r[1] = s[1];
}

// Cache policy of the conv kernels' OUTPUT stores (the aux operand of buffer_store: bit 0 sc0, bit 1 nt, bit 4 sc1).  The outputs of a
// conv are not read again by the same launch, while its INPUT lines are (a k-step fetches 32 bytes of a 128-byte line, the other k-steps
// and the neighbouring tiles want the rest): stores that allocate in L2 could push those lines out.  Measured in round 5
// (profiles/r05_ab_e7_store_policy.txt; make alt NAME=st2 EXTRA=-DLP_OUT_STORE_AUX=2): non-temporal stores make the
// batch-8 step 4 % SLOWER (79.7 against 76.5 ms; sc0+nt and nt+sc1 the same or worse) and the inference forward 3 % -- the default stays 0.
#ifndef LP_OUT_STORE_AUX
#define LP_OUT_STORE_AUX 0
#endif

// GroupNorm-apply on the way IN: the conv reads the RAW output c of the previous conv and applies a = relu((c - mean) rstd gamma + beta)
// (group_norm.py:110-122 + the ReLU of resnet.py:133-136) to each input plane after it has landed in LDS -- inference only, where no
// backward needs the applied tensor: the 1 read + 1 write pass of bts_lp_gn_apply goes away.  Slab semantics with whole z planes per
// group (D % G == 0) and classes that tile a 16-byte slot (cg | 8): a slot's eight channels then have classes e mod cg whatever the slot.
// The arithmetic is bts_lp_gn_apply's, element for element (max(fmaf(v - mean, rstd * gamma, beta), 0), rounded to the storage type).
struct LpGnaFuse {
  const float* gamma;
  const float* beta;
  const float* mean;   // (N*G)
  const float* rstd;
  int G, cg;
};

// the arithmetic of the GNA transforms on one 16-byte slot: o = max(fmaf(v - mu, sc, be), 0) per element, rounded to the storage type --
// on the packed fp32 instructions (v_pk_add_f32 / v_pk_fma_f32: the same IEEE results as the scalar forms bts_lp_gn_apply uses)
template <typename T> __device__ __forceinline__ u32x4 lp_gna_slot(u32x4 raw, float mu, const float (&sc)[8], const float (&be)[8]) {
  const f32x2_ m2 = {mu, mu};
  u32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f32x2_ v = {T::ld((unsigned short)(raw[k] & 0xffffu)), T::ld((unsigned short)(raw[k] >> 16))};
    const f32x2_ t = __builtin_elementwise_fma(v - m2, f32x2_{sc[2 * k], sc[2 * k + 1]}, f32x2_{be[2 * k], be[2 * k + 1]});
    r[k] = pack2<T>(fmaxf(t[0], 0.f), fmaxf(t[1], 0.f));
  }
  return r;
}

// GroupNorm-backward class sums from the epilogue of the data-gradient conv that PRODUCES the GroupNorm output's gradient (resnet.py:80-93
// under train.py:151: conv2^T(dc2) = da, then GN1 backward needs A_j = sum da_E * xh and B_j = sum da_E per (sample, group, class
// j = channel mod cg) before anything else -- lp_gn_bwd_reduce_kernel's pass over da and c1).  The epilogue holds da in registers; it
// reads the matching 16 bytes of the GroupNorm INPUT x per stored 16 bytes and leaves the class sums as per-(unit, slot) partial rows
// in lp_gn_bwd_finalize_kernel's layout [N*G][B][cg][2] (fp64).  Slab semantics (whole z planes per group: D % G == 0).
struct LpGnbFuse {
  const unsigned short* x;   // GroupNorm input, dense (N, D, H, W, C) with C = the conv's output channels here
  const float* gamma;
  const float* beta;
  const float* mean;         // [N*G]
  const float* rstd;
  double* part;              // [N*G][B][cg][2]
  int G, cg, relu;
  long B;
};

// ---- shared block arithmetic of the non-conv passes (lowp_norm.hip, lowp_block.hip; tests/lowp_ref.py restates it) ----
// Chunks of one (sample, slab) unit of Lu elements for the chunked apply kernels: enough workgroups for ~16 per CU, at least 4 iterations
// each where the unit is that long.  Returns the elements per chunk, *B = chunks per unit.
inline long lp_chunk_per(long Lu, long units, int* B, long target = 4096) {
  const long steps = Lu / 2048;                 // 2048-element steps of a unit
  long b = target / units;
  if (b > steps / 4) b = steps / 4;
  if (b < 1) b = 1;
  const long per = (steps + b - 1) / b;
  *B = (int)((steps + per - 1) / per);
  return per * 2048;
}
// reduce-pass workgroups per (sample, group) unit of L elements of the GroupNorm backward and the fused block backward
inline int lp_gnb_blocks(long L) {
  long b = L / (2048 * 16);
  if (b < 1) b = 1;
  if (b > 256) b = 256;
  return (int)b;
}
// The tiling of lp_gn_bwd_reduce / apply and of the fused block backward's kernels: whole 2048-element steps per (sample, group) unit,
// a power-of-two C <= 256, classes (cg = C / G) that tile a 256-thread workgroup and fit the reduce pass's four lanes per wave.
// Outside it bts_lp_gn_bwd and bts_lp_block_bwd answer BTS_ERR_UNSUPPORTED (their argument checks come first and answer BTS_ERR_SHAPE).
inline bool lp_gn_bwd_tiled(long V, int C, int G) {
  if (V <= 0 || G <= 0 || C < G) return false;
  const long E = V * C, L = E / G;
  const int cg = C / G;
  return E % G == 0 && L % 2048 == 0 && cg <= 32 && 256 % cg == 0 && C <= 256 && (C & (C - 1)) == 0;
}

// ---- stride-1 3x3x3 convolutions: which of the three kernels takes a call (lowp_s1z.hip, lowp_s1d.hip, lowp.hip's register-staged
// lp_conv_s1_kernel), decided ONCE per query or launch by lp_s1_choose; the workspace queries and the entry points answer from it ----
struct LpS1Call {         // shape, strides (elements) and requested form of one call -- no pointers
  int N, D, H, W, Cin, ldx, Cout, ldy;
  int accum;
  int G;                  // GroupNorm partial sums of y, slab mode, G groups (0: none) -- an epilogue: it does not change the choice
  int gnb_G;              // GroupNorm-backward class sums in the epilogue (LpGnbFuse::G; 0: none) -- likewise
  int gna_G;              // GroupNorm + ReLU applied to the input planes (LpGnaFuse::G; 0: none)
  int ldx2;               // SC: voxel stride of the centre-tap second operand (0: none)
  int Cout2, ldy2;        // FS: shortcut output columns and their voxel stride (0: none)
  long ysplit;            // split output: elements between the tensors of consecutive 32-column blocks (0: one tensor)
  int ldxb;               // channels [32, 64) of a 64-channel input as a tensor of their own, voxel stride ldxb (0: none)
  int aligned;            // every operand sits on a 16-byte boundary
};
struct S1zPlan { int ntx, nty, nzc, ZC, nitems, ipw, nwg, xcd, pair; };      // pair: Cin = 64 as two 32-channel passes
struct S1dPlan {
  int mode, txl, ntx, nty, ntz, ncg, ksplit, ks_per;
  int bx, by, bz;
  long nitems;
};
struct LpS1Shape { int vb, cb, txl, ntx, nty, ntz, ncg, ksplit, ks_per; long wgs; };      // the register-staged kernel
enum { LP_S1Z = 1, LP_S1D, LP_S1 };
struct LpS1Choice {
  int kernel;             // LP_S1Z | LP_S1D | LP_S1
  S1zPlan z;
  S1dPlan d;
  LpS1Shape s;
  long ws;                // conv workspace bytes (split-K partial sums)
  long B;                 // GroupNorm partial slots per (n, group) the kernel writes for LpS1Call::G / gnb_G; 0: it cannot
};
struct LpS1Ptrs {         // the operands of a launch (NULL: absent); wp = the whole K3S1 image
  const void* x;
  const void* wp;
  const float* bias;
  void* y;
  void* ws;
  long ws_bytes;
  double* gnp;            // [N*G][B][2] (LpS1Call::G)
  const LpGnbFuse* gb;
  const LpGnaFuse* ga;
  const void* x2;         // SC
  const void* wp2;        // SC / FS: the K1 image
  void* y2;               // FS
  const float* bias2;
  double* gap_part;
  const void* xb;         // LpS1Call::ldxb
};
// true: the kernel takes the call (every shape, stride and form condition of its launcher; which kernel has which form is
// lp_s1_choose's rule) -- ch's plan, ws and B are filled in, and the launcher does not decline it
bool lp_s1z_accept(const LpS1Call& c, LpS1Choice& ch);
bool lp_s1d_accept(const LpS1Call& c, LpS1Choice& ch);
bool lp_s1_accept(const LpS1Call& c, LpS1Choice& ch);
// BTS_OK: ch = the call's kernel.  1: no kernel takes the operand form asked for (SC, FS, gna, ysplit, ldxb); ch = the choice of the same
// call without it.  Otherwise the status of a call no kernel takes.
int lp_s1_choose(const LpS1Call& c, LpS1Choice& ch);
inline bool lp_s1_same(const LpS1Choice& a, const LpS1Choice& b) { return a.kernel == b.kernel && a.ws == b.ws && a.B == b.B; }
// the query's view of a call: dense strides, aligned operands
inline LpS1Call lp_s1_call(int N, int D, int H, int W, int Cin, int Cout) {
  LpS1Call c{};
  c.N = N; c.D = D; c.H = H; c.W = W; c.Cin = Cin; c.ldx = Cin; c.Cout = Cout; c.ldy = Cout;
  c.aligned = 1;
  return c;
}
// lowp.hip: launch ch's kernel (q.wp = the whole K3S1 image)
int lp_s1_run(int dtype, const LpS1Call& c, const LpS1Choice& ch, LpS1Ptrs q, hipStream_t stream);
inline long lp_s1z_fs_B(const S1zPlan& pl) { return (long)pl.ntx * pl.nty * pl.nzc * 8; }      // FS column-sum rows per sample
int bts_lp_s1z_launch_(int dtype, const LpS1Call& c, const LpS1Choice& ch, const LpS1Ptrs& q, hipStream_t stream);     // q.wp = the DMA part
int bts_lp_s1d_launch_(int dtype, const LpS1Call& c, const LpS1Choice& ch, const LpS1Ptrs& q, hipStream_t stream);
// lowp_s1d.hip: the DMA part of a K3S1 image -- its bytes, and packing it at dst
long bts_lp_s1d_image_bytes_(int K, int N);
int bts_lp_s1d_pack_(int dtype, const LpPackParams& p, void* dst, hipStream_t stream);
// lowp.hip: the finish of a split-K launch, y (+)= round(bias + sum_z part[z]) in fixed order; the _gn_ form also leaves the slab-mode
// GroupNorm partials of the rounded y, bts_lp_splitk_gn_B_ slots per (n, group) (0: it does not take the shape)
long bts_lp_splitk_gn_B_(int N, long V, int Cout, int G);
int bts_lp_splitk_reduce_gn_(int dtype, const float* part, const float* bias, void* y, double* gn_partial, int N, long V, int Cout, int G,
                             int ksplit, hipStream_t stream);
int bts_lp_splitk_reduce_(int dtype, const float* part, const float* bias, void* y, long nvox, int Cout, int Npad, int ldy, int ksplit,
                          int accum, hipStream_t stream);

// ---- 1x1x1, stride-2 and transposed convolutions and the data gradients on those geometries: which kernel takes a call (lowp_k1.hip,
// lowp_s2t.hip, lowp_up.hip, else lowp_gather.hip), decided ONCE per query or launch by lp_g_choose; queries and entry points answer from it ----
struct LpGCall {          // geometry, shape, strides (elements) and requested form of one call -- no pointers
  int geo;                // 0 = 1x1x1, 2 = stride-2 gather (out = ceil(in/2)), 3 = the 8 output-parity classes of the transposed form (out = 2 in)
  int N, D, H, W, Cin, ldx, Cout, ldy, accum;      // (D, H, W: the tensor the taps read)
  int want_gap;           // geo 0: column sums of the unrounded output as partial rows [sample][row][Cout] (the squeeze)
  int G;                  // geo 3: GroupNorm partial sums of the fine output, slab mode, G groups (0: none)
  int x16, wp16, y_al;    // x / the weight image on a 16-byte boundary; y on 16 | 8 (the streaming and the merged kernel store 16 bytes), 0: neither
};
struct K1Plan { int lf, cb, ncg, nit; long blocks; };      // lf: lp_k1f_kernel (whole 128-byte row pieces); nit: 256-position blocks per workgroup
struct S2tPlan { int ntx, nty, ntz; long ntiles; };
struct UpPlan { int mode, txl, ntx, nty, ntz, ncg; long nitems; };
struct LpGatherPlan { int vb, cb, gk, ncg; long npos, blocks; };      // gk: 0 = lp_conv_gather_kernel<vb, cb>, 2 | 4 = lp_conv_gatherq_kernel<cb, gk[, vb]>
enum { LP_G_K1 = 1, LP_G_S2T, LP_G_UP, LP_G_GATHER };
struct LpGChoice {
  int kernel;             // LP_G_K1 | LP_G_S2T | LP_G_UP | LP_G_GATHER (geo 3: eight launches of the one plan)
  union { K1Plan k; S2tPlan t; UpPlan u; LpGatherPlan g; };      // the plan of `kernel`
  long rows;              // partial rows the kernel writes: per sample for want_gap, per (n, group) for G; 0: it cannot, or none asked for
};
// the operands of a launch (NULL: absent); wp = the whole image, part = the partial rows: [N][rows][Cout] (want_gap) | [N*G][rows][2] (G)
struct LpGPtrs { const void *x, *wp; const float* bias; void* y; double* part; };
// the A/B switches of the family (BTS_LP_K1 | UP | S2T | GATHERQ = 0: the kernel is off and the gather kernels take its calls): read per call
inline bool lp_switch_on(const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); }
// true: the kernel takes the call (every switch, shape, stride, alignment and 31-bit condition of its launcher) -- its plan and rows are
// filled in, and the launcher does not decline it.  Which geometry goes to which kernel is lp_g_choose's rule.
bool lp_k1_accept(const LpGCall& c, LpGChoice& ch);
bool lp_s2t_accept(const LpGCall& c, LpGChoice& ch);
bool lp_up_accept(const LpGCall& c, LpGChoice& ch);
bool lp_gather_accept(const LpGCall& c, LpGChoice& ch);
// BTS_OK: ch = the call's kernel; rows = 0 where no kernel emits the partials asked for (ch = the choice of the plain call then: the
// caller forms them from the stored result).  Otherwise the status of a call no kernel takes.
int lp_g_choose(const LpGCall& c, LpGChoice& ch);
int bts_lp_k1_launch_(int dtype, const LpGCall& c, const LpGChoice& ch, const LpGPtrs& q, hipStream_t stream);
int bts_lp_s2t_launch_(int dtype, const LpGCall& c, const LpGChoice& ch, const LpGPtrs& q, hipStream_t stream);
int bts_lp_up_launch_(int dtype, const LpGCall& c, const LpGChoice& ch, const LpGPtrs& q, hipStream_t stream);
// One call of the family (c's alignment flags come from q): chosen, put through the common argument check and launched.  q->part holds
// max_rows partial rows; partials that would not fit are not asked for.  q == NULL: the query's view, aligned operands, the choice only.
int bts_lp_g_conv_(int dtype, LpGCall c, const LpGPtrs* q, long max_rows, LpGChoice& ch, hipStream_t stream);
// lowp_block.hip: out[n][c] = scale * the sum of the B partial rows [n][b][c], fixed order
int bts_lp_colsum_finalize_(const double* partial, float* out, int N, int C, int B, double scale, hipStream_t stream);
// lowp_point.hip: db[c] (+)= the sum of the nblocks partial rows part[b][c] of row length C, block order, c < ncols (lp_dbias_finalize_kernel)
int bts_lp_dbias_finalize_(const double* part, float* db, int ncols, int nblocks, int C, int accum, hipStream_t stream);

// byte offset of the DMA part inside a K3S1 / K3S2T-forward / K3S2-data-gradient image with K contraction channels and N output columns
inline long lp_s1d_part_offset(int K, int N) { return 27L * ((K + 15) / 16) * ((N + 31) / 32) * 1024; }
inline bool lp_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// what every conv launch checks before it looks at the geometry
inline int lp_conv_check(int dtype, const void* x, const void* wp, const void* y, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return BTS_ERR_SHAPE;
  // (results are stored four couts = 8 bytes at a time; a head with fewer than four output channels stores them one by one)
  const bool vec_out = Cout >= 4;
  if (Cin % 16 != 0 || ldx % 8 != 0 || (vec_out && ldy % 4 != 0) || ldx < Cin || ldy < Cout) return BTS_ERR_ALIGN;
  if (!lp_al16(x) || (((uintptr_t)y) & (vec_out ? 7 : 1)) || !lp_al16(wp)) return BTS_ERR_ALIGN;
  return BTS_OK;
}

// ---- 16-bit weight gradients: which of the three kernels takes a call (the streaming lp_wgd_kernel of lowp_wgd.hip, the general LDS-tiled
// lp_wgrad_kernel of lowp_wg.hip, the strided lp_wgs_kernel of lowp_wgs.hip) and where its workspace areas lie, decided ONCE per query or
// launch by lp_wg_choose; the workspace queries and the entry points answer from it ----
struct LpWgCall {         // kind, shape, strides (elements) and requested form of one call -- no pointers
  int kind, N, D, H, W, Cin, ldx, Cout, lddy;      // (D, H, W: the forward-input grid x lives on)
  int dup_start, dup_shift, accum;
  int want_db;            // db (+)= the column sums of dy is asked for
  int gna_G;              // GNA: x is the RAW input of a GroupNorm (+ ReLU) of gna_G groups, applied to the P planes in LDS (0: none)
  int k1f, lddy1;         // K1F: the 1x1x1 weight gradient of a second conv on the same input, from dy1 with voxel stride lddy1
  long x_split;           // x as a list of 32-channel tensors x + b * x_split with voxel stride ldx (0: one tensor)
  int aligned;            // every operand and the workspace sit on a 16-byte boundary
};
struct WgdPlan { int ntx, nty, nzc, ZC, nitems, ipw, nwg, ncp, ncq, xcd; };
struct LpWgPlan { int nq, nwg, ncp, ncqg, ntx, nty, ntz; long ntiles; };      // the general and the strided kernel
enum { LP_WGD = 1, LP_WG, LP_WGS };
struct LpWgChoice {
  int kernel;             // LP_WGD | LP_WG | LP_WGS (0: none)
  WgdPlan d;
  LpWgPlan g;
  long part;              // bytes of the partial-slab area at the head of the workspace (a whole number of 4 KB slabs)
  long cs_off, cws_off;   // byte offsets of the per-sample column sums of dy and of bts_lp_colsum's workspace behind it
  long ws;                // the whole workspace
};
// the operands of a launch (NULL: absent); ga: LpWgCall::gna_G, dy1 / dw1: LpWgCall::k1f
struct LpWgPtrs { const void *x, *dy; float* dw; void* ws; const LpGnaFuse* ga; const void* dy1; float* dw1; };
// the general and the strided kernel: persistent 512-thread workgroups over nz x ny x nx tiles per sample, one per CU over the whole launch
inline void lp_wg_tiles(LpWgPlan& g, int N, int Cp, int Cq, int nx, int ny, int nz) {
  g.nq = Cq >= 64 ? 2 : 1;
  g.ncp = (Cp + 31) / 32;
  g.ncqg = (Cq + 32 * g.nq - 1) / (32 * g.nq);
  g.ntx = nx; g.nty = ny; g.ntz = nz;
  g.ntiles = (long)N * nz * ny * nx;
  const long per = (long)g.ncp * g.ncqg, cap = per < 256 ? 256 / per : 1;
  g.nwg = (int)(g.ntiles < cap ? g.ntiles : cap);
}
// voxels per sample of the grid dy lives on: the half grid of a stride-2 conv, the doubled grid of a transposed one
inline long lp_wg_dy_voxels(const LpWgCall& c) {
  if (c.kind == BTS_CONV_K3S2) return (long)(c.D / 2) * (c.H / 2) * (c.W / 2);
  return (c.kind == BTS_CONV_K3S2T ? 8L : 1L) * c.D * c.H * c.W;
}
// true: the kernel takes the call (every shape, stride, 31-bit offset and form condition of its launcher) -- ch's kernel, plan and part are
// filled in, and the launcher does not decline it
bool lp_wgd_accept(const LpWgCall& c, LpWgChoice& ch);      // K3S1, every form
bool lp_wg_accept(const LpWgCall& c, LpWgChoice& ch);       // K3S1 and K1, no form
bool lp_wgs_accept(const LpWgCall& c, LpWgChoice& ch);      // K3S2 and K3S2T
// BTS_OK: ch = the call's kernel and workspace layout, and the launch cannot fail on its arguments any more.  1: the streaming kernel does
// not take the form asked for (GNA, K1F, x_split).  Otherwise the status of the call; ch is still filled in wherever a kernel could be
// planned (the sizing query answers for every channel count).
int lp_wg_choose(const LpWgCall& c, LpWgChoice& ch);
int bts_lp_wgd_launch_(int dtype, const LpWgCall& c, const LpWgChoice& ch, const LpWgPtrs& q, hipStream_t stream);
int bts_lp_wgs_launch_(int dtype, const LpWgCall& c, const LpWgChoice& ch, const LpWgPtrs& q, hipStream_t stream);
// lowp_wg.hip: dw (+)= the partial slabs summed in fixed order (layout [workgroup][cp block][cq group][slot][32][32 * NQ]), fold included
int bts_lp_wgrad_finalize_(const float* part, float* dw, int nwg, int ncp, int ncqg, int nslot, int ntaps, int NQ, int Cp, int Cq, int Cin_ref,
                           int dup_start, int dup_shift, int accum, hipStream_t stream);
