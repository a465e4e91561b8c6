// Transposed-conv gather form with all 8 output-parity classes in ONE workgroup (Conv3DTranspose k3 s2 forward,
// upsample.py:28-33, and the data gradient of the stride-2 conv, downsample.py:28-35).
// out[2c+p] = sum over the taps of parity class p of in[c+d] * W[k]  with per axis  p=0: (k,d) in {(0,0),(2,-1)}, p=1: (1,0).
// The per-class launches of igemm_kernel give the 1-,2- and 4-tap classes 8..32 MFMAs per staged 8-channel slab, far too
// little to cover staging and barriers (51-62 TF).  Here a wave owns 32 coarse voxels and ALL 8 classes: 8 accumulators,
// the 27 taps of a slab need only the 8 input fragments at offsets {-1,0}^3 (8 ds_read_b128 for 108 MFMAs), and the
// tap -> (class, offset) map is compile-time.
#include <stdlib.h>
#include "common.h"
#include "conv_plan.h"

#define UPM_NSLOT 3
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
  float* part;     // split-K partials [ksplit][fine voxel][Npad] (bts_igemm_reduce_ finishes them)
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
bool upm_accept(const ConvCall& c, ConvChoice& ch) {
  UpmPlan& u = ch.u;
  if ((c.ldx & 3) || (c.ldy & 3) || !c.x16 || !c.y16) return false;
  if ((c.Cin & 7) || (c.Cout & 3) || c.Wi < 8 || c.Hi < 4 || c.Di < 2) return false;
  const int Npad = conv_npad32(c.Cout), KG = c.Cin / 8;
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
  ch.sym = SYM_UPM;
  ch.ws = u.need;
  return c.ws_bytes >= u.need;
}

int bts_upm_launch_(const ConvCall& c, const ConvChoice& ch, const ConvPtrs& q, hipStream_t stream) {
  const UpmPlan& u = ch.u;
  UpmParams p;
  p.N = c.N; p.Di = c.Di; p.Hi = c.Hi; p.Wi = c.Wi; p.Cin = c.Cin; p.Cout = c.Cout;
  p.Npad = conv_npad32(c.Cout); p.KG = c.Cin / 8;
  p.lgTX = u.lgTX; p.lgTY = u.lgTY; p.TZ = u.TZ; p.ntx = u.ntx; p.nty = u.nty; p.ntz = u.ntz; p.IX = u.IX; p.IY = u.IY; p.IZ = u.IZ;
  p.ksplit = u.ksplit; p.kg_per = u.kg_per;
  p.x = q.x; p.wp = q.wp; p.bias = q.bias; p.y = q.y; p.ldx = c.ldx; p.ldy = c.ldy; p.flags = c.flags;
  p.part = reinterpret_cast<float*>(q.ws);
  const long tiles = (long)c.N * p.ntz * p.nty * p.ntx;
  const int ny = p.Npad / 32;
  const int tileVox = p.IZ * p.IY * p.IX;
  const size_t shmem = (size_t)2 * tileVox * 12 * sizeof(float);
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(ch.sym, 2.0 * 27.0 * c.Cin * c.Cout * (double)c.N * c.Di * c.Hi * c.Wi, stream);
  (void)hipGetLastError(); hipLaunchKernelGGL(upm_kernel, dim3((unsigned)tiles, ny, p.ksplit), dim3(256), shmem, stream, p);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  if (p.ksplit <= 1) return BTS_OK;
  return bts_igemm_reduce_(p.part, q.bias, q.y, (long)c.N * 8 * c.Di * c.Hi * c.Wi, c.Cout, p.Npad, c.ldy, p.ksplit, p.flags, stream);
}
