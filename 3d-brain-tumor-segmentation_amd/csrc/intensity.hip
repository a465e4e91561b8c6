// Intensity augmentation of an augmented batch on the device: Gaussian noise, Gaussian blur, brightness, contrast, gamma (the
// nnU-Net / batchgenerators set; semantics in include/bts_hip.h above bts_intensity_batch).
// The unit of work is a JOB: one (example n, channel c) volume of vol = T0*T1*T2 voxels that has the stage's flag set.  Voxel t of a job
// lives at x[((n*vol + t)*C + c)] (layout 0) or x[(n*C + c)*vol + t] (layout 1); everything below is written in terms of (job, t), so
// the two layouts, any N and any split into launches give the same bits.  A launch carries up to INT_JOBS_MAX jobs by value.
// Passes (each a launch over the jobs that need it; a job with no flag is in no table and is never written):
//   noise   x -> x                                   v = fmaf(s, z, v)
//   blur    x -> ws (axis 2), ws -> x (axis 1), x -> ws (axis 0); every later pass of the job reads ws ("src") until `apply A` stores to x
//   stats A src*m  -> (mu, sd, lo, hi)               [contrast]
//   apply A src -> x                                 [blur | brightness | contrast]   b = v*m;  o = clip(fmaf(b - mu, f, mu), lo, hi)
//   stats B +-x -> (mu, sd, lo, hi)                  [gamma]    (+-: the invert flag)
//   apply B x -> x                                   [gamma]    y = +-v;  o = fmaf(powf((y - lo) / ((hi - lo) + 1e-7f), g), hi - lo, lo)
//   stats C x -> (mu', sd')                          [gamma]
//   apply C x -> x                                   [gamma]    o = +-fmaf((v - mu') / (sd' + 1e-8f), sd, mu)
// Statistics: a job's voxels are dealt to nb = min(INT_STAT_BLOCKS, ceil(vol / 256)) blocks (nb depends on vol alone), thread i of
// block b takes t = b*256 + i, + nb*256, ...; fp64 sums of d = g(v) - pivot and d*d (pivot = g of voxel 0, so a constant volume sums
// exact zeros), exact fp32 min / max; wave, block and the nb partials are combined in a fixed order.  mu = (float)(pivot + S/vol),
// sd = (float)sqrt(max(Q/vol - (S/vol)^2, 0)).  No atomics.
// No fp contraction in this file: the products and sums round as written (the tolerance of tests/test_intensity_host.py restates them).
#include <cmath>
#include "common.h"
#include "bts_internal.h"

#pragma clang fp contract(off)

#define INT_MAXC 16
#define INT_MAXR 16
#define INT_JOBS_MAX 32
#define INT_STAT_BLOCKS 64

#define INT_NOISE 1
#define INT_BLUR 2
#define INT_BRIGHT 4
#define INT_CONTRAST 8
#define INT_GAMMA 16
#define INT_INVERT 32

struct IntJob {
  int n, c;
  int r;             // blur radius
  int mode;          // apply passes: the job's flags; stats: 1 = read ws
  uint32_t k0, k1;   // noise key
  float p0, p1;      // noise: s | stats: the factor g(v) = v * p0 | apply A: m, f | apply B: gamma
  float w[INT_MAXR + 1];   // blur weights w[|j|]
  float pad;
};
struct IntLaunch {
  float* x;          // the batch
  float* ws;         // blur scratch, laid out like x
  double* part;      // [n*C + c][INT_STAT_BLOCKS][4]: S, Q, min, max of the statistics pass in flight
  float* fin;        // [n*C + c][4]: mu, sd, lo, hi; the region this statistics pass finalizes into
  long vol;
  int C, T0, T1, T2, layout, njobs, nb, axis, pass;
  IntJob j[INT_JOBS_MAX];
};

// A job's volume starts at int_base() (block-uniform: scalar arithmetic) and its voxel t sits t * int_stride() floats further on; the
// entry point refuses vol * C >= 2^31, so offsets inside a volume are 32-bit
__device__ __forceinline__ long int_base(const IntLaunch& p, const IntJob& j) {
  return p.layout == 0 ? (long)j.n * p.vol * p.C + j.c : ((long)j.n * p.C + j.c) * p.vol;
}
__device__ __forceinline__ int int_stride(const IntLaunch& p) { return p.layout == 0 ? p.C : 1; }

// Philox4x32-10 (Salmon et al. 2011): counter (c0,c1,c2,c3), key (k0,k1)
__device__ __forceinline__ void int_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
  for (int i = 0; i < 10; ++i) {
    const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(b >> 32) ^ c1 ^ k0, n1 = (uint32_t)b, n2 = (uint32_t)(a >> 32) ^ c3 ^ k1, n3 = (uint32_t)a;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// blocks are numbered job-fastest (blockIdx.x = chunk * njobs + job): the channels of an example, interleaved in a channels-last
// batch, are swept side by side and share their cache lines in L2
__global__ __launch_bounds__(256) void intensity_noise_kernel(const IntLaunch p) {
  const IntJob& j = p.j[blockIdx.x % p.njobs];
  const int t = (int)(blockIdx.x / p.njobs) * 256 + threadIdx.x;
  if (t >= p.vol) return;
  const uint64_t e = (uint64_t)t * p.C + j.c, q = e >> 2;
  uint32_t o[4];
  int_philox((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, j.k0, j.k1, o);
  const int k = (int)(e & 3);
  const uint32_t wa = (k & 2) ? o[2] : o[0], wb = (k & 2) ? o[3] : o[1];
  const float u1 = (float)((wa >> 8) + 1u) * (1.0f / 16777216.0f), u2 = (float)(wb >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u1)), ang = 6.283185307179586f * u2;
  const float z = r * ((k & 1) ? sinf(ang) : cosf(ang));
  float* a = p.x + int_base(p, j) + t * int_stride(p);
  *a = __builtin_fmaf(j.p0, z, *a);
}

// scipy.ndimage mode='reflect' (d c b a | a b c d | d c b a), period 2n
__device__ __forceinline__ int int_reflect(int i, int n) {
  const int per = 2 * n;
  int m = i % per;
  if (m < 0) m += per;
  return m < n ? m : per - 1 - m;
}

// one axis of the separable blur: out[t] = sum_{j=-r..r} w[|j|] * in[reflect(t_axis + j)], fmaf chain from 0 in the order j = -r..r
__global__ __launch_bounds__(256) void intensity_blur_kernel(const IntLaunch p) {
  const IntJob& j = p.j[blockIdx.x % p.njobs];
  const int t = (int)(blockIdx.x / p.njobs) * 256 + threadIdx.x;
  if (t >= p.vol) return;
  const long base = int_base(p, j);
  const float* src = ((p.axis == 1) ? p.ws : p.x) + base;
  float* dst = ((p.axis == 1) ? p.x : p.ws) + base;
  const int st = int_stride(p);
  int pos, ext, step;      // the voxel's index along the axis, the axis' extent, and its stride in voxels
  if (p.axis == 2) { pos = (unsigned)t % (unsigned)p.T2; ext = p.T2; step = 1; }
  else if (p.axis == 1) { pos = ((unsigned)t / (unsigned)p.T2) % (unsigned)p.T1; ext = p.T1; step = p.T2; }
  else { step = p.T1 * p.T2; pos = (unsigned)t / (unsigned)step; ext = p.T0; }
  const int r = j.r;
  float acc = 0.f;
  const int line = t - pos * step;
  if (r < ext) {
    // one reflection at the most, without a branch: along axis 2 every wave holds border voxels, and a separate interior path would
    // make it run both (four taps' loads are in flight at once; the sum keeps its order)
#pragma unroll 4
    for (int k = -r; k <= r; ++k) {
      int i = pos + k;
      i = i < 0 ? -1 - i : i;
      i = i >= ext ? 2 * ext - 1 - i : i;
      acc = __builtin_fmaf(j.w[k < 0 ? -k : k], src[(line + i * step) * st], acc);
    }
  } else {
    for (int k = -r; k <= r; ++k) acc = __builtin_fmaf(j.w[k < 0 ? -k : k], src[(line + int_reflect(pos + k, ext) * step) * st], acc);
  }
  dst[t * st] = acc;
}

__global__ __launch_bounds__(256) void intensity_stats_kernel(const IntLaunch p) {
  __shared__ double sh[4];
  __shared__ float shm[8];
  const IntJob& j = p.j[blockIdx.x % p.njobs];
  const int b = blockIdx.x / p.njobs;
  const float* src = (j.mode ? p.ws : p.x) + int_base(p, j);
  const int st = int_stride(p);
  const float pv = src[0] * j.p0;
  double s = 0.0, q = 0.0;
  float mn = pv, mx = pv;
  for (int t = b * 256 + threadIdx.x; t < p.vol; t += p.nb * 256) {
    const float v = src[t * st] * j.p0;
    const double d = (double)v - (double)pv;
    s += d; q += d * d;
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  const double bs = block_sum_f64(s, sh), bq = block_sum_f64(q, sh);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { shm[threadIdx.x >> 6] = mn; shm[4 + (threadIdx.x >> 6)] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { mn = fminf(mn, shm[i]); mx = fmaxf(mx, shm[4 + i]); }
    double* d = p.part + ((long)j.n * p.C + j.c) * INT_STAT_BLOCKS * 4 + (long)b * 4;
    d[0] = bs; d[1] = bq; d[2] = (double)mn; d[3] = (double)mx;
  }
}

// one wave per job: the nb partials in the order of their blocks
__global__ __launch_bounds__(64) void intensity_finalize_kernel(const IntLaunch p) {
  if (threadIdx.x != 0) return;
  const IntJob& j = p.j[blockIdx.x];
  const float* src = (j.mode ? p.ws : p.x) + int_base(p, j);
  const double pv = (double)(src[0] * j.p0);
  const double* d = p.part + ((long)j.n * p.C + j.c) * INT_STAT_BLOCKS * 4;
  double s = 0.0, q = 0.0, mn = d[2], mx = d[3];
  for (int b = 0; b < p.nb; ++b) { s += d[4 * b]; q += d[4 * b + 1]; mn = fmin(mn, d[4 * b + 2]); mx = fmax(mx, d[4 * b + 3]); }
  const double m = s / (double)p.vol;
  double var = q / (double)p.vol - m * m;
  if (var < 0.0) var = 0.0;
  float* f = p.fin + ((long)j.n * p.C + j.c) * 4;
  f[0] = (float)(pv + m); f[1] = (float)sqrt(var); f[2] = (float)mn; f[3] = (float)mx;
}

// pass 0 = apply A, 1 = apply B, 2 = apply C (see the head of the file); fin0 / fin1: the two regions of final statistics
__global__ __launch_bounds__(256) void intensity_apply_kernel(const IntLaunch p, const float* fin0, const float* fin1) {
  const IntJob& j = p.j[blockIdx.x % p.njobs];
  const int t = (int)(blockIdx.x / p.njobs) * 256 + threadIdx.x;
  if (t >= p.vol) return;
  const long a = int_base(p, j) + t * int_stride(p), jf = ((long)j.n * p.C + j.c) * 4;
  if (p.pass == 0) {
    float v = ((j.mode & INT_BLUR) ? p.ws : p.x)[a];
    if (j.mode & INT_BRIGHT) v = v * j.p0;
    if (j.mode & INT_CONTRAST) {
      const float mu = fin0[jf], lo = fin0[jf + 2], hi = fin0[jf + 3];
      v = fminf(fmaxf(__builtin_fmaf(v - mu, j.p1, mu), lo), hi);
    }
    p.x[a] = v;
  } else if (p.pass == 1) {
    const float lo = fin1[jf + 2], R = fin1[jf + 3] - lo;
    const float y = (j.mode & INT_INVERT) ? -p.x[a] : p.x[a];
    p.x[a] = __builtin_fmaf(powf((y - lo) / (R + 1e-7f), j.p0), R, lo);
  } else {
    const float mu = fin1[jf], sd = fin1[jf + 1], mu2 = fin0[jf], sd2 = fin0[jf + 1];
    const float o = __builtin_fmaf((p.x[a] - mu2) / (sd2 + 1e-8f), sd, mu);
    p.x[a] = (j.mode & INT_INVERT) ? -o : o;
  }
}

static long int_round256(long b) { return (b + 255) / 256 * 256; }

extern "C" long bts_intensity_batch_workspace(int N, int T0, int T1, int T2, int C) {
  if (N <= 0 || C <= 0 || C > INT_MAXC || T0 <= 0 || T1 <= 0 || T2 <= 0) return BTS_ERR_SHAPE;
  const long nc = (long)N * C;
  return int_round256((long)T0 * T1 * T2 * nc * (long)sizeof(float)) + int_round256(nc * INT_STAT_BLOCKS * 4 * (long)sizeof(double)) +
         int_round256(2 * nc * 4 * (long)sizeof(float));
}

extern "C" long bts_intensity_blur_weights(float sigma, float* weights) {
  if (!(sigma > 0.f) || !std::isfinite(sigma)) return BTS_ERR_SHAPE;
  const double sd = (double)sigma;
  const long r = (long)(4.0 * sd + 0.5);
  if (r > INT_MAXR) return BTS_ERR_SHAPE;
  double w[INT_MAXR + 1], sum = 0.0;
  // scipy.ndimage._filters._gaussian_kernel1d: exp(-0.5 / sigma^2 * j^2) over j = -r..r, divided by its sum (summed in that order)
  for (long k = -r; k <= r; ++k) { const double e = std::exp(-0.5 / (sd * sd) * (double)(k * k)); if (k >= 0) w[k] = e; sum += e; }
  if (weights)
    for (long k = 0; k <= r; ++k) weights[k] = (float)(w[k] / sum);
  return r;
}

extern "C" int bts_intensity_batch(float* x, int N, int T0, int T1, int T2, int C, int layout, const int* flags, const float* params,
                                   const uint32_t* keys, void* workspace, long workspace_bytes, hipStream_t stream) {
  if (N <= 0 || C <= 0 || C > INT_MAXC || T0 <= 0 || T1 <= 0 || T2 <= 0 || (layout != 0 && layout != 1)) return BTS_ERR_SHAPE;
  if (x == nullptr || flags == nullptr || params == nullptr || keys == nullptr) return BTS_ERR_SHAPE;
  if (workspace == nullptr || workspace_bytes < bts_intensity_batch_workspace(N, T0, T1, T2, C)) return BTS_ERR_SHAPE;
  const long nc = (long)N * C, vol = (long)T0 * T1 * T2;
  if (vol * C > 0x7fffffffL - 256 * 65) return BTS_ERR_SHAPE;      // (offsets inside a volume, and the statistics' loop index, are 32-bit)
  int any = 0;
  for (long i = 0; i < nc; ++i) {
    const int f = flags[i];
    const float* q = params + 5 * i;      // s, sigma, m, f, gamma
    if (f & ~63) return BTS_ERR_SHAPE;
    if ((f & INT_NOISE) && !(std::isfinite(q[0]) && q[0] >= 0.f)) return BTS_ERR_SHAPE;
    if ((f & INT_BLUR) && bts_intensity_blur_weights(q[1], nullptr) < 0) return BTS_ERR_SHAPE;
    if ((f & INT_BRIGHT) && !(std::isfinite(q[2]) && q[2] > 0.f)) return BTS_ERR_SHAPE;
    if ((f & INT_CONTRAST) && !(std::isfinite(q[3]) && q[3] > 0.f)) return BTS_ERR_SHAPE;
    if ((f & INT_GAMMA) && !(std::isfinite(q[4]) && q[4] > 0.f)) return BTS_ERR_SHAPE;
    any |= f & 31;
  }
  if (!any) return BTS_OK;
  IntLaunch p;
  char* w = reinterpret_cast<char*>(workspace);
  p.x = x; p.ws = reinterpret_cast<float*>(w);
  w += int_round256(vol * nc * (long)sizeof(float));
  p.part = reinterpret_cast<double*>(w);
  w += int_round256(nc * INT_STAT_BLOCKS * 4 * (long)sizeof(double));
  float* fin0 = reinterpret_cast<float*>(w);
  float* fin1 = fin0 + nc * 4;
  p.fin = fin0; p.axis = 0; p.pass = 0; p.njobs = 0;
  p.vol = vol; p.C = C; p.T0 = T0; p.T1 = T1; p.T2 = T2; p.layout = layout;
  const long chunks = (vol + 255) / 256;
  p.nb = (int)(chunks < INT_STAT_BLOCKS ? chunks : INT_STAT_BLOCKS);

  // the passes in order; each gathers the jobs that need it and launches them INT_JOBS_MAX at a time
  enum { NOISE, BLUR2, BLUR1, BLUR0, STATA, APPLYA, STATB, APPLYB, STATC, APPLYC, NPASS };
  for (int pass = 0; pass < NPASS; ++pass) {
    p.njobs = 0;
    for (long i = 0; i <= nc; ++i) {
      if (i < nc) {
        const int f = flags[i];
        const float* q = params + 5 * i;
        bool want;
        switch (pass) {
          case NOISE: want = f & INT_NOISE; break;
          case BLUR2: case BLUR1: case BLUR0: want = f & INT_BLUR; break;
          case STATA: want = f & INT_CONTRAST; break;
          case APPLYA: want = f & (INT_BLUR | INT_BRIGHT | INT_CONTRAST); break;
          default: want = f & INT_GAMMA; break;
        }
        if (want) {
          IntJob& j = p.j[p.njobs++];
          j.n = (int)(i / C); j.c = (int)(i % C); j.r = 0; j.mode = f; j.k0 = keys[2 * j.n]; j.k1 = keys[2 * j.n + 1];
          j.p0 = 0.f; j.p1 = 0.f; j.pad = 0.f;
          for (int k = 0; k <= INT_MAXR; ++k) j.w[k] = 0.f;
          switch (pass) {
            case NOISE: j.p0 = q[0]; break;
            case BLUR2: case BLUR1: case BLUR0: j.r = (int)bts_intensity_blur_weights(q[1], j.w); break;
            case STATA: j.mode = (f & INT_BLUR) ? 1 : 0; j.p0 = (f & INT_BRIGHT) ? q[2] : 1.f; break;
            case APPLYA: j.p0 = q[2]; j.p1 = q[3]; break;
            case STATB: j.mode = 0; j.p0 = (f & INT_INVERT) ? -1.f : 1.f; break;
            case APPLYB: j.p0 = q[4]; break;
            case STATC: j.mode = 0; j.p0 = 1.f; break;
            default: break;
          }
        }
      }
      if (p.njobs == INT_JOBS_MAX || (i == nc && p.njobs > 0)) {
        const unsigned grid = (unsigned)(chunks * p.njobs);
        (void)hipGetLastError();
        if (pass == NOISE) hipLaunchKernelGGL(intensity_noise_kernel, dim3(grid), dim3(256), 0, stream, p);
        else if (pass == BLUR2 || pass == BLUR1 || pass == BLUR0) {
          p.axis = pass == BLUR2 ? 2 : pass == BLUR1 ? 1 : 0;
          hipLaunchKernelGGL(intensity_blur_kernel, dim3(grid), dim3(256), 0, stream, p);
        } else if (pass == STATA || pass == STATB || pass == STATC) {
          p.fin = pass == STATB ? fin1 : fin0;
          hipLaunchKernelGGL(intensity_stats_kernel, dim3((unsigned)(p.nb * p.njobs)), dim3(256), 0, stream, p);
          BTS_LAUNCH_CHECK();
          hipLaunchKernelGGL(intensity_finalize_kernel, dim3((unsigned)p.njobs), dim3(64), 0, stream, p);
        } else {
          p.pass = pass == APPLYA ? 0 : pass == APPLYB ? 1 : 2;
          hipLaunchKernelGGL(intensity_apply_kernel, dim3(grid), dim3(256), 0, stream, p, (const float*)fin0, (const float*)fin1);
        }
        BTS_LAUNCH_CHECK();
        p.njobs = 0;
      }
    }
  }
  return BTS_OK;
}
