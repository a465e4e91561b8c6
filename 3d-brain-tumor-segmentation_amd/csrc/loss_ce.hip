// Compound training loss (no reference counterpart; gfx950, ONE streaming pass per entry point): the Dice + VAE loss of loss.hip:2 plus
// a voxel-wise cross-entropy / focal term on the head's fused sigmoid p (fp32) and the target t in [0,1]:
//   q    = min(max(p, EPS), 1 - EPS), EPS = 2^-23 (both bounds exact in fp32)
//   e    = w_pos t (1-q)^gamma (-log q) + w_neg (1-t) q^gamma (-log(1-q))        gamma = 0: binary cross-entropy; alpha: w_pos = alpha,
//   CE   = sum(e) / (N_global V C)                                                 w_neg = 1 - alpha
//   loss = w_dice dice + w_ce CE + 0.1 l2 + 0.1 kl                                 (dice, l2, kl: loss.hip:2, batch summed into I, P, T)
// The raw sums of a batch shard add over the shards (all-reduce them between bts_seg_loss_sums and bts_seg_loss_value, like loss.hip's).
//
// OPERATION ORDER, all fp32, a * b * c read left to right, no division in the through-sigmoid form (tests/loss_ce_ref.py restates it):
//   om = 1 - q;  lq = logf(q);  l1 = logf(om);  a = w_pos * t;  b = w_neg * (1 - t)
//   term (sums):   gamma = 0:  e = a * (-lq) + b * (-l1)
//                  gamma > 0:  pa = pw(om, gamma); pb = pw(q, gamma);  e = a * pa * (-lq) + b * pb * (-l1)
//                              pw(b, gamma) = b * b * ... * b (gamma factors, left to right) for gamma = 1, 2, ..., 8 -- the default 2 is
//                              one product -- and powf(b, gamma) otherwise (two powf per element are 2-3 x the time of the whole pass:
//                              DESIGN.md, "Compound loss"; expf(gamma * l) would reuse the logarithms but multiplies their rounding by
//                              |gamma l|, up to 100 eps32 in the tails)
//                  e is added to the channel's fp64 accumulator (fp64 lives in the accumulators only)
//   gradient of e with respect to the logit, d e / d q * q (1 - q) (zero where p < EPS or p > 1 - EPS: the clamp's derivative; q = p inside):
//                  gamma = 0:  pos = -om;                          neg = q                     (w_pos = w_neg = w: s = w (p - t))
//                  gamma > 0:  pos = pa * (gamma * q * lq - om);   neg = pb * (q - gamma * om * l1)       (no cancellation in either;
//                              pa, pb as in the sums)
//                              with l1 = log1pf(-q) HERE: for small q, logf(1 - q) carries the rounding of 1 - q, eps32 / q relative to
//                              l1 ~ -q, and gamma om l1 is as large as the q it is added to (the sums pay for that rounding in their
//                              bound, a gradient element cannot)
//                  s = a * pos + b * neg;   without through_sigmoid (d e / d q itself): s = s / (q * om)
//   dlogit = dice gradient of loss.hip:114 with w_dice folded into k1, k2  +  kce * s,   kce = (float)(w_ce / (count C) * gscale),
//   count = sums[4C+4] (the global N V after the all-reduce).  dyvae, dproj: loss.hip:115.
#include <cfloat>
#include "common.h"
#include "bts_internal.h"

#define LOSS_MAXC 8          // = loss.hip's (the Python side sizes nothing by it; the sums layouts below depend on C alone)
#define LOSS_BLOCKS 1024     // = loss.hip's grid cap of the partial-sum pass; the backward's is 4096 as there
#define SEG_NACC (4 * LOSS_MAXC + 1)
#define SEG_EPS 1.1920928955078125e-07f      // 2^-23
#define SEG_MAX_GAMMA 8.0f

static bool seg_weight_ok(float w) { return w >= 0.f && w <= FLT_MAX; }      // false for NaN, Inf and negatives
static bool seg_gamma_ok(float g) { return g >= 0.f && g <= SEG_MAX_GAMMA; }
// kernel instantiation: 0 = binary cross-entropy (no power), 1 = gamma in {1, ..., 8} (products), 2 = any other gamma (powf)
static int seg_mode(float gamma) { return gamma == 0.f ? 0 : (gamma == floorf(gamma) ? 1 : 2); }
template <int MODE> __device__ __forceinline__ float seg_pw(float b, float gamma) {
  if (MODE == 2) return powf(b, gamma);
  float r = b;
  for (int i = 1; i < (int)gamma; ++i) r *= b;      // wave-uniform trip count
  return r;
}
static int seg_shape_check(int N, long V, int C, int ldp, int ldy, bool vae, int Cx, int ldx, int ldv, int Lz) {
  if (N <= 0 || V <= 0 || C <= 0 || C > LOSS_MAXC || ldp < C || ldy < C || Lz < 0) return BTS_ERR_SHAPE;
  if (vae && (Cx <= 0 || ldx < Cx || ldv < Cx)) return BTS_ERR_SHAPE;
  return BTS_OK;
}

// partial layout per block: [0..MAXC) I, [MAXC..2MAXC) P, [2MAXC..3MAXC) T, [3MAXC] sum (x-y_vae)^2, [3MAXC+1..4MAXC+1) sum e
template <int MODE>
__global__ __launch_bounds__(256) void seg_loss_partial_kernel(const float* __restrict__ ypred, const float* __restrict__ y,
                                                               const float* __restrict__ x, const float* __restrict__ yvae,
                                                               double* partial, long NV, int C, int ldp, int ldy, int Cx, int ldx,
                                                               int ldv, float gamma, float wpos, float wneg) {
  __shared__ double sh[8];
  double acc[SEG_NACC];
#pragma unroll
  for (int i = 0; i < SEG_NACC; ++i) acc[i] = 0.0;
  for (long v = blockIdx.x * (long)blockDim.x + threadIdx.x; v < NV; v += (long)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < LOSS_MAXC; ++c)
      if (c < C) {
        const float p = ypred[v * ldp + c], t = y[v * ldy + c];
        acc[c] += (double)(p * t);
        acc[LOSS_MAXC + c] += (double)(p * p);
        acc[2 * LOSS_MAXC + c] += (double)(t * t);
        const float q = fminf(fmaxf(p, SEG_EPS), 1.f - SEG_EPS);
        const float om = 1.f - q, lq = logf(q), l1 = logf(om);
        float a = wpos * t, b = wneg * (1.f - t);
        if (MODE) {
          a *= seg_pw<MODE>(om, gamma);
          b *= seg_pw<MODE>(q, gamma);
        }
        acc[3 * LOSS_MAXC + 1 + c] += (double)(a * (-lq) + b * (-l1));
      }
    if (x) {
      float m = 0.f;
      for (int c = 0; c < Cx; ++c) {
        const float d = x[v * ldx + c] - yvae[v * ldv + c];
        m = fmaf(d, d, m);
      }
      acc[3 * LOSS_MAXC] += (double)m;
    }
  }
#pragma unroll      // (a runtime index would move acc[] to scratch memory)
  for (int i = 0; i < SEG_NACC; ++i) {
    const double r = block_sum_f64(acc[i], sh);
    if (threadIdx.x == 0) partial[(long)blockIdx.x * SEG_NACC + i] = r;
  }
}

// sums layout (double): [0, 3C+4) as loss.hip:14, [3C+4, 4C+4) sum e per channel, [4C+4] this shard's N*V
__global__ void seg_loss_finalize_kernel(const double* partial, const float* proj, double* sums, int blocks, int C, int N, int Lz,
                                         double numel_x, double count) {
  __shared__ double sh[8];
  for (int i = 0; i < 4 * C + 1; ++i) {
    int src, dst;
    if (i < 3 * C) { src = (i / C) * LOSS_MAXC + (i % C); dst = i; }
    else if (i == 3 * C) { src = 3 * LOSS_MAXC; dst = i; }
    else { src = 3 * LOSS_MAXC + 1 + (i - 3 * C - 1); dst = i + 3; }
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += blockDim.x) s += partial[(long)b * SEG_NACC + src];
    const double r = block_sum_f64(s, sh);
    if (threadIdx.x == 0) sums[dst] = r;
  }
  double k = 0.0;
  if (proj)
    for (int i = threadIdx.x; i < N * Lz; i += blockDim.x) {
      const int n = i / Lz, j = i % Lz;
      const float mu = proj[n * 2 * Lz + j], lv = proj[n * 2 * Lz + Lz + j];
      k += (double)(mu * mu + expf(lv) - lv - 1.0f);
    }
  const double rk = block_sum_f64(k, sh);
  if (threadIdx.x == 0) {
    sums[3 * C + 1] = rk;
    sums[3 * C + 2] = numel_x;
    sums[3 * C + 3] = (double)N * Lz;
    sums[4 * C + 4] = count;
  }
}

extern "C" long bts_seg_loss_workspace(void) { return (long)LOSS_BLOCKS * SEG_NACC * 8 + 64; }

// Raw sums of this rank's batch shard -> sums[4C+5] (double, device). x/y_vae/proj may be null (no VAE terms).
extern "C" int bts_seg_loss_sums(const float* y_pred, const float* y, const float* x, const float* y_vae, const float* proj,
                                 double* sums, void* workspace, long workspace_bytes, int N, long V, int C, int ldp, int ldy, int Cx,
                                 int ldx, int ldv, int Lz, float gamma, float w_pos, float w_neg, hipStream_t stream) {
  const int r = seg_shape_check(N, V, C, ldp, ldy, x != nullptr, Cx, ldx, ldv, Lz);
  if (r != BTS_OK) return r;
  if (!seg_gamma_ok(gamma) || !seg_weight_ok(w_pos) || !seg_weight_ok(w_neg)) return BTS_ERR_UNSUPPORTED;
  if (workspace_bytes < bts_seg_loss_workspace()) return BTS_ERR_WORKSPACE;
  const long NV = (long)N * V;
  long blocks = (NV + 255) / 256;
  if (blocks > LOSS_BLOCKS) blocks = LOSS_BLOCKS;
  double* partial = reinterpret_cast<double*>(workspace);
  (void)hipGetLastError();
  const int mode = seg_mode(gamma);
  auto kernel = mode == 0 ? seg_loss_partial_kernel<0> : (mode == 1 ? seg_loss_partial_kernel<1> : seg_loss_partial_kernel<2>);
  hipLaunchKernelGGL(kernel, dim3((int)blocks), dim3(256), 0, stream, y_pred, y, x, y_vae, partial, NV, C, ldp, ldy, Cx, ldx, ldv, gamma,
                     w_pos, w_neg);
  BTS_LAUNCH_CHECK();
  (void)hipGetLastError();
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, stream, partial, proj, sums, (int)blocks, C, N, Lz,
                     x ? (double)NV * Cx : 0.0, (double)NV);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// loss (1 float) and its four components {dice, l2, kl, ce} from (possibly all-reduced) sums
__global__ void seg_loss_value_kernel(const double* sums, float* loss, float* parts, int C, int has_vae, float w_dice, float w_ce) {
  if (threadIdx.x || blockIdx.x) return;
  double d = 0.0, ce = 0.0;
  for (int c = 0; c < C; ++c) {
    d += 1.0 - (2.0 * sums[c] + 1.0) / (sums[C + c] + sums[2 * C + c] + 1.0);
    ce += sums[3 * C + 4 + c];
  }
  d /= C;
  ce /= sums[4 * C + 4] * C;
  double l2 = 0.0, kl = 0.0;
  if (has_vae) {
    l2 = sums[3 * C] / sums[3 * C + 2];
    kl = sums[3 * C + 1] / sums[3 * C + 3];
  }
  loss[0] = (float)((double)w_dice * d + (double)w_ce * ce + 0.1 * l2 + 0.1 * kl);
  if (parts) { parts[0] = (float)d; parts[1] = (float)l2; parts[2] = (float)kl; parts[3] = (float)ce; }
}
extern "C" int bts_seg_loss_value(const double* sums, float* loss, float* parts, int C, int has_vae, float w_dice, float w_ce,
                                  hipStream_t stream) {
  if (C <= 0 || C > LOSS_MAXC) return BTS_ERR_SHAPE;
  if (!seg_weight_ok(w_dice) || !seg_weight_ok(w_ce)) return BTS_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  hipLaunchKernelGGL(seg_loss_value_kernel, dim3(1), dim3(64), 0, stream, sums, loss, parts, C, has_vae, w_dice, w_ce);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

template <int MODE>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ ypred, const float* __restrict__ y,
                                                           const float* __restrict__ x, const float* __restrict__ yvae,
                                                           const float* __restrict__ proj, const double* __restrict__ sums,
                                                           const float* __restrict__ gscale, float* __restrict__ dlogit,
                                                           float* __restrict__ dyvae, float* __restrict__ dproj, long NV, int C,
                                                           int ldp, int ldy, int Cx, int ldx, int ldv, int N, int Lz,
                                                           int through_sigmoid, float w_dice, float w_ce, float gamma, float wpos,
                                                           float wneg) {
  const float gs = gscale ? gscale[0] : 1.f;
  float k1[LOSS_MAXC], k2[LOSS_MAXC];
#pragma unroll
  for (int c = 0; c < LOSS_MAXC; ++c) {
    k1[c] = k2[c] = 0.f;
    if (c < C) {
      const double D = sums[C + c] + sums[2 * C + c] + 1.0;
      k1[c] = (float)(-2.0 / (C * D) * gs * w_dice);
      k2[c] = (float)(2.0 * (2.0 * sums[c] + 1.0) / (C * D * D) * gs * w_dice);
    }
  }
  const float kce = (float)((double)w_ce / (sums[4 * C + 4] * C) * gs);
  const float kx = x ? (float)(0.2 / sums[3 * C + 2]) * gs : 0.f;
  for (long v = blockIdx.x * (long)blockDim.x + threadIdx.x; v < NV; v += (long)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < LOSS_MAXC; ++c)
      if (c < C) {
        const float p = ypred[v * ldp + c], t = y[v * ldy + c];
        float g = k1[c] * t + k2[c] * p;
        if (through_sigmoid) g *= p * (1.f - p);
        // the clamp's derivative: 0 strictly outside [EPS, 1 - EPS]; q stays inside for the logarithms, the result is then dropped
        const bool inside = p >= SEG_EPS && p <= 1.f - SEG_EPS;
        const float q = fminf(fmaxf(p, SEG_EPS), 1.f - SEG_EPS);
        const float om = 1.f - q;
        float pos = -om, neg = q;
        if (MODE) {
          const float lq = logf(q), l1 = log1pf(-q);
          pos = seg_pw<MODE>(om, gamma) * (gamma * q * lq - om);
          neg = seg_pw<MODE>(q, gamma) * (q - gamma * om * l1);
        }
        float s = wpos * t * pos + wneg * (1.f - t) * neg;
        if (!through_sigmoid) s = s / (q * om);
        dlogit[v * C + c] = inside ? g + kce * s : g;
      }
    if (x)
      for (int c = 0; c < Cx; ++c) dyvae[v * Cx + c] = kx * (yvae[v * ldv + c] - x[v * ldx + c]);
  }
  if (proj && blockIdx.x == 0) {
    const float kz = (float)(1.0 / sums[3 * C + 3]) * gs;
    for (int i = threadIdx.x; i < N * Lz; i += blockDim.x) {
      const int n = i / Lz, j = i % Lz;
      dproj[n * 2 * Lz + j] = 0.2f * kz * proj[n * 2 * Lz + j];
      dproj[n * 2 * Lz + Lz + j] = 0.1f * kz * (expf(proj[n * 2 * Lz + Lz + j]) - 1.f);
    }
  }
}
extern "C" int bts_seg_loss_bwd(const float* y_pred, const float* y, const float* x, const float* y_vae, const float* proj,
                                const double* sums, const float* gscale, float* dlogit, float* dyvae, float* dproj, int N, long V,
                                int C, int ldp, int ldy, int Cx, int ldx, int ldv, int Lz, int through_sigmoid, float w_dice,
                                float w_ce, float gamma, float w_pos, float w_neg, hipStream_t stream) {
  const int r = seg_shape_check(N, V, C, ldp, ldy, x != nullptr, Cx, ldx, ldv, Lz);
  if (r != BTS_OK) return r;
  if (!seg_gamma_ok(gamma) || !seg_weight_ok(w_pos) || !seg_weight_ok(w_neg) || !seg_weight_ok(w_dice) || !seg_weight_ok(w_ce))
    return BTS_ERR_UNSUPPORTED;
  const long NV = (long)N * V;
  long blocks = (NV + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  (void)hipGetLastError();
  const int mode = seg_mode(gamma);      // 0: s = w_pos t (q - 1) + w_neg (1 - t) q, no logarithm and no power
  auto kernel = mode == 0 ? seg_loss_bwd_kernel<0> : (mode == 1 ? seg_loss_bwd_kernel<1> : seg_loss_bwd_kernel<2>);
  hipLaunchKernelGGL(kernel, dim3((int)blocks), dim3(256), 0, stream, y_pred, y, x, y_vae, proj, sums, gscale, dlogit, dyvae, dproj, NV, C,
                     ldp, ldy, Cx, ldx, ldv, N, Lz, through_sigmoid, w_dice, w_ce, gamma, w_pos, w_neg);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
