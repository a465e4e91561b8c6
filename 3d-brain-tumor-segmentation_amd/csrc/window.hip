// Sliding-window inference: the three passes around the forwards of a windowed TestTimeAugmentor.
//   window_gather      cut B windows out of the raw volume, zero beyond its end, normalise and flip each in the same pass (the windowed form
//                      of pad + normalise + tf.reverse, test.py:107,128-148,164-178)
//   window_accumulate  un-flip B predictions and add them, weighted by the separable importance tables, into the accumulator (test.py:139-151
//                      with a window's weight in place of 1/count alone)
//   window_occupancy   brain-mask voxels per window, so that windows on empty space are not run at all
// Dense fp32 tensors, channels innermost.  The job table (window starts, flips, table rows, per-job mean and std) travels by value in the
// kernel arguments, WIN_MAXB jobs per launch.  Plain HIP C++: whole 16-byte accesses where the addresses allow, integer atomics only in
// the occupancy count, no float atomics anywhere.
#include "common.h"
#include "bts_internal.h"

#define WIN_MAXB 16
#define WIN_MAXC 16
#define WIN_GRID_Y 32768

struct WinJobs {
  int n;
  int z0[WIN_MAXB], y0[WIN_MAXB], x0[WIN_MAXB], flip[WIN_MAXB];
  int iz[WIN_MAXB], iy[WIN_MAXB], ix[WIN_MAXB];   // rows of the three importance tables (accumulate only)
};
struct WinNorm { float mean[WIN_MAXB][WIN_MAXC], stdv[WIN_MAXB][WIN_MAXC]; };

__device__ __forceinline__ bool win_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// n4 16-byte accesses; the caller has checked the alignment
template <int N4> __device__ __forceinline__ void win_ld(const float* p, float (&r)[4 * N4]) {
#pragma unroll
  for (int q = 0; q < N4; ++q) {
    const f32x4 t = reinterpret_cast<const f32x4*>(p)[q];
    r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w;
  }
}
template <int N4> __device__ __forceinline__ void win_st(float* p, const float (&r)[4 * N4]) {
#pragma unroll
  for (int q = 0; q < N4; ++q) reinterpret_cast<f32x4*>(p)[q] = f32x4{r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]};
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------
// out[b, od, oh, ow, c] = (v - mean_b[c]) / std_b[c], v = x[z0 + fd(od), y0 + fh(oh), x0 + fw(ow), c] inside the volume and 0 beyond its
// end (the reference pads the raw intensities before it normalises them).  CT = C in 1..4: a thread owns four consecutive OUTPUT voxels of
// a row, 4 C floats = C 16-byte stores; their four source voxels are consecutive too (reversed under a W flip), C 16-byte loads, and the
// voxels are reversed in registers.  A group at the volume's end, in a short tail or on misaligned addresses goes voxel by voxel.  CT = 0:
// any C up to WIN_MAXC, one voxel per thread.  blockIdx.y walks the (job, od) planes, so a thread finds its row with one 32-bit division.
template <int CT>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ x, float* __restrict__ out, WinJobs jobs, WinNorm nrm,
                                                            int D, int H, int W, int C, int R0, int R1, int R2) {
  constexpr int G = CT > 0 ? 4 : 1;
  const int Cc = CT > 0 ? CT : C;
  const int ng = (R2 + G - 1) / G;
  const int per_plane = R1 * ng;
  const int nplanes = jobs.n * R0;
  for (int plane = blockIdx.y; plane < nplanes; plane += gridDim.y) {
    const int b = plane / R0, od = plane - b * R0;
    const int fl = jobs.flip[b];
    const int z = jobs.z0[b] + ((fl & 4) ? R0 - 1 - od : od);
    const int x0 = jobs.x0[b];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per_plane; i += gridDim.x * 256) {
      const int oh = i / ng, ow = (i - oh * ng) * G;
      const int y = jobs.y0[b] + ((fl & 2) ? R1 - 1 - oh : oh);
      const int nv = R2 - ow < G ? R2 - ow : G;
      float* o = out + (((long)plane * R1 + oh) * R2 + ow) * Cc;
      const bool row_in = z < D && y < H;
      const float* xrow = row_in ? x + ((long)z * H + y) * W * Cc : x;
      if constexpr (CT > 0) {
        const int xlo = x0 + ((fl & 1) ? R2 - 4 - ow : ow);             // the lowest of the four source voxels (>= x0 when nv == 4)
        const float* s = xrow + (long)xlo * CT;
        if (nv == 4 && row_in && xlo + 3 < W && win_al16(s) && win_al16(o)) {
          float r[4 * CT], q[4 * CT];
          win_ld<CT>(s, r);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int c = 0; c < CT; ++c) q[j * CT + c] = (r[((fl & 1) ? 3 - j : j) * CT + c] - nrm.mean[b][c]) / nrm.stdv[b][c];
          }
          win_st<CT>(o, q);
          continue;
        }
      }
      for (int j = 0; j < nv; ++j) {
        const int xs = x0 + ((fl & 1) ? R2 - 1 - (ow + j) : ow + j);
        const bool in = row_in && xs < W;
        for (int c = 0; c < Cc; ++c) {
          const float v = in ? xrow[(long)xs * Cc + c] : 0.f;
          o[j * Cc + c] = (v - nrm.mean[b][c]) / nrm.stdv[b][c];
        }
      }
    }
  }
}

static int win_check_jobs(int B, const int* starts, const int* flips, int D, int H, int W) {
  if (B < 1 || B > WIN_MAXB) return BTS_ERR_UNSUPPORTED;
  if (starts == nullptr || flips == nullptr) return BTS_ERR_SHAPE;
  for (int b = 0; b < B; ++b) {
    if (flips[b] & ~7) return BTS_ERR_SHAPE;
    if (starts[3 * b] < 0 || starts[3 * b] >= D || starts[3 * b + 1] < 0 || starts[3 * b + 1] >= H || starts[3 * b + 2] < 0 ||
        starts[3 * b + 2] >= W)
      return BTS_ERR_SHAPE;
  }
  return BTS_OK;
}
// in-row and in-plane indices are int, and a start plus a window extent must not wrap
static bool win_fits(int D, int H, int W, int C, int R0, int R1, int R2) {
  const long big = 0x3fffffffL;
  return (long)W * C <= big && ((long)R2 + 4) * C <= big && (long)R1 * ((R2 + 3) / 4 + 1) <= big && (long)WIN_MAXB * R0 <= big &&
         (long)D + R0 <= big && (long)H + R1 <= big && (long)W + R2 <= big;
}

extern "C" long bts_window_batch_max(void) { return WIN_MAXB; }

extern "C" int bts_window_gather(const float* x, float* out, int D, int H, int W, int C, int R0, int R1, int R2, int B, const int* starts,
                                 const int* flips, const float* mean, const float* stdv, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || C <= 0 || R0 <= 0 || R1 <= 0 || R2 <= 0) return BTS_ERR_SHAPE;
  if (C > WIN_MAXC) return BTS_ERR_UNSUPPORTED;
  if (!win_fits(D, H, W, C, R0, R1, R2)) return BTS_ERR_SHAPE;
  const int st = win_check_jobs(B, starts, flips, D, H, W);
  if (st != BTS_OK) return st;
  if (mean == nullptr || stdv == nullptr) return BTS_ERR_SHAPE;
  WinJobs jobs = {};
  WinNorm nrm = {};
  jobs.n = B;
  for (int b = 0; b < B; ++b) {
    jobs.z0[b] = starts[3 * b]; jobs.y0[b] = starts[3 * b + 1]; jobs.x0[b] = starts[3 * b + 2]; jobs.flip[b] = flips[b];
    for (int c = 0; c < C; ++c) { nrm.mean[b][c] = mean[b * C + c]; nrm.stdv[b][c] = stdv[b * C + c]; }
  }
  const int G = C <= 4 ? 4 : 1;
  const long per_plane = (long)R1 * ((R2 + G - 1) / G);
  long gx = (per_plane + 255) / 256;
  if (gx > 4096) gx = 4096;
  long gy = (long)B * R0;
  if (gy > WIN_GRID_Y) gy = WIN_GRID_Y;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
  (void)hipGetLastError();
  switch (C) {
    case 1: hipLaunchKernelGGL(window_gather_kernel<1>, grid, block, 0, stream, x, out, jobs, nrm, D, H, W, C, R0, R1, R2); break;
    case 2: hipLaunchKernelGGL(window_gather_kernel<2>, grid, block, 0, stream, x, out, jobs, nrm, D, H, W, C, R0, R1, R2); break;
    case 3: hipLaunchKernelGGL(window_gather_kernel<3>, grid, block, 0, stream, x, out, jobs, nrm, D, H, W, C, R0, R1, R2); break;
    case 4: hipLaunchKernelGGL(window_gather_kernel<4>, grid, block, 0, stream, x, out, jobs, nrm, D, H, W, C, R0, R1, R2); break;
    default: hipLaunchKernelGGL(window_gather_kernel<0>, grid, block, 0, stream, x, out, jobs, nrm, D, H, W, C, R0, R1, R2); break;
  }
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------------
// Owner computes: a thread owns four consecutive accumulator voxels of a row (KT = K in 1..4; one voxel for KT = 0) inside the bounding
// box of the launch's windows, reads them once, walks the jobs IN LIST ORDER, adds every job whose window holds the voxel and writes the
// touched voxels once.  Nothing else writes them in this launch, so overlapping jobs need no atomics and the order of the additions is
// the job order whatever B is.  Per value: w = ((scale * nz[d]) * ny[h]) * nx[w'], then acc = acc + w * pred, each product and the sum
// rounded on its own (the pragma below forbids the contraction into an fma): B jobs in one launch and one job in each of B launches give
// the same bits.  Groups are aligned to four voxels of the ACCUMULATOR row; a prediction's four voxels are consecutive as well (reversed
// under a W flip).  A group at a window's edge or at the row's end goes voxel by voxel.
template <int KT>
__global__ __launch_bounds__(256) void window_accumulate_kernel(const float* __restrict__ pred, float* acc, const float* __restrict__ nz,
                                                                const float* __restrict__ ny, const float* __restrict__ nx, WinJobs jobs,
                                                                int bz0, int by0, int gx0, int nbz, int nby, int ngx, int H, int W, int K,
                                                                int R0, int R1, int R2, float scale) {
#pragma clang fp contract(off)
  constexpr int G = KT > 0 ? 4 : 1;
  constexpr int KV = KT > 0 ? KT : 1;
  const int Kc = KT > 0 ? KT : K;
  const int per_plane = nby * ngx;
  for (int pz = blockIdx.y; pz < nbz; pz += gridDim.y) {
    const int z = bz0 + pz;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per_plane; i += gridDim.x * 256) {
      const int yy = i / ngx;
      const int y = by0 + yy, w0 = (gx0 + (i - yy * ngx)) * G;
      const int nv = W - w0 < G ? W - w0 : G;
      float* a = acc + (((long)z * H + y) * W + w0) * Kc;
      if constexpr (KT > 0) {
        float v[4 * KV];
        unsigned touched = 0u;
        bool loaded = false;
        const bool avec = nv == 4 && win_al16(a);
        for (int b = 0; b < jobs.n; ++b) {
          const int d = z - jobs.z0[b], h = y - jobs.y0[b], wl0 = w0 - jobs.x0[b];
          if ((unsigned)d >= (unsigned)R0 || (unsigned)h >= (unsigned)R1 || wl0 + nv <= 0 || wl0 >= R2) continue;
          if (!loaded) {
            loaded = true;
            if (avec) win_ld<KV>(a, v);
            else {
#pragma unroll
              for (int e = 0; e < 4 * KV; ++e) v[e] = e < nv * KV ? a[e] : 0.f;
            }
          }
          const int fl = jobs.flip[b];
          const int sd = (fl & 4) ? R0 - 1 - d : d, sh = (fl & 2) ? R1 - 1 - h : h;
          const float t = (scale * nz[(long)jobs.iz[b] * R0 + d]) * ny[(long)jobs.iy[b] * R1 + h];
          const float* prow = pred + (((long)b * R0 + sd) * R1 + sh) * R2 * KV;
          const float* nxr = nx + (long)jobs.ix[b] * R2;
          if (nv == 4 && wl0 >= 0 && wl0 + 3 < R2) {
            const float* s = prow + (long)((fl & 1) ? R2 - 4 - wl0 : wl0) * KV;
            float r[4 * KV];
            if (win_al16(s)) win_ld<KV>(s, r);
            else {
#pragma unroll
              for (int e = 0; e < 4 * KV; ++e) r[e] = s[e];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float wv = t * nxr[wl0 + j];
#pragma unroll
              for (int k = 0; k < KV; ++k) {
                const float term = wv * r[((fl & 1) ? 3 - j : j) * KV + k];
                v[j * KV + k] = v[j * KV + k] + term;
              }
            }
            touched = 15u;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int wl = wl0 + j;
              if (j < nv && (unsigned)wl < (unsigned)R2) {
                const float wv = t * nxr[wl];
                const float* s = prow + (long)((fl & 1) ? R2 - 1 - wl : wl) * KV;
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                  const float term = wv * s[k];
                  v[j * KV + k] = v[j * KV + k] + term;
                }
                touched |= 1u << j;
              }
            }
          }
        }
        if (touched == 0u) continue;
        if (touched == 15u && avec) win_st<KV>(a, v);
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (touched & (1u << j)) {
#pragma unroll
              for (int k = 0; k < KV; ++k) a[j * KV + k] = v[j * KV + k];
            }
          }
        }
      } else {
        for (int k = 0; k < Kc; ++k) {
          float v = 0.f;
          bool loaded = false;
          for (int b = 0; b < jobs.n; ++b) {
            const int d = z - jobs.z0[b], h = y - jobs.y0[b], wl = w0 - jobs.x0[b];
            if ((unsigned)d >= (unsigned)R0 || (unsigned)h >= (unsigned)R1 || (unsigned)wl >= (unsigned)R2) continue;
            if (!loaded) { loaded = true; v = a[k]; }
            const int fl = jobs.flip[b];
            const int sd = (fl & 4) ? R0 - 1 - d : d, sh = (fl & 2) ? R1 - 1 - h : h, sw = (fl & 1) ? R2 - 1 - wl : wl;
            const float t = (scale * nz[(long)jobs.iz[b] * R0 + d]) * ny[(long)jobs.iy[b] * R1 + h];
            const float wv = t * nx[(long)jobs.ix[b] * R2 + wl];
            const float term = wv * pred[((((long)b * R0 + sd) * R1 + sh) * R2 + sw) * Kc + k];
            v = v + term;
          }
          if (loaded) a[k] = v;
        }
      }
    }
  }
}

extern "C" int bts_window_accumulate(const float* pred, float* acc, const float* nz, const float* ny, const float* nx, int n0, int n1,
                                     int n2, int D, int H, int W, int K, int R0, int R1, int R2, int B, const int* starts, const int* flips,
                                     const int* rows, float scale, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || K <= 0 || R0 <= 0 || R1 <= 0 || R2 <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0) return BTS_ERR_SHAPE;
  if (!win_fits(D, H, W, K, R0, R1, R2) || (long)H * ((W + 3) / 4 + 1) > 0x3fffffffL) return BTS_ERR_SHAPE;
  const int st = win_check_jobs(B, starts, flips, D, H, W);
  if (st != BTS_OK) return st;
  if (rows == nullptr) return BTS_ERR_SHAPE;
  for (int b = 0; b < B; ++b)
    if (rows[3 * b] < 0 || rows[3 * b] >= n0 || rows[3 * b + 1] < 0 || rows[3 * b + 1] >= n1 || rows[3 * b + 2] < 0 || rows[3 * b + 2] >= n2)
      return BTS_ERR_SHAPE;
  {  // the owner of an accumulator voxel reads predictions other owners never write: the two buffers must not share a byte
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(pred), a0 = reinterpret_cast<uintptr_t>(acc);
    const uintptr_t p1 = p0 + (uintptr_t)B * R0 * R1 * R2 * K * sizeof(float), a1 = a0 + (uintptr_t)D * H * W * K * sizeof(float);
    if (p0 < a1 && a0 < p1) return BTS_ERR_UNSUPPORTED;
  }
  WinJobs jobs = {};
  jobs.n = B;
  int lo[3] = {D, H, W}, hi[3] = {0, 0, 0};
  const int ext[3] = {D, H, W}, roi[3] = {R0, R1, R2};
  for (int b = 0; b < B; ++b) {
    jobs.z0[b] = starts[3 * b]; jobs.y0[b] = starts[3 * b + 1]; jobs.x0[b] = starts[3 * b + 2]; jobs.flip[b] = flips[b];
    jobs.iz[b] = rows[3 * b]; jobs.iy[b] = rows[3 * b + 1]; jobs.ix[b] = rows[3 * b + 2];
    for (int a = 0; a < 3; ++a) {
      const int s = starts[3 * b + a];
      const int e = s + roi[a] < ext[a] ? s + roi[a] : ext[a];
      if (s < lo[a]) lo[a] = s;
      if (e > hi[a]) hi[a] = e;
    }
  }
  const int G = K <= 4 ? 4 : 1;
  const int gx0 = lo[2] / G, ngx = (hi[2] + G - 1) / G - gx0, nbz = hi[0] - lo[0], nby = hi[1] - lo[1];
  long gx = ((long)nby * ngx + 255) / 256;
  if (gx > 4096) gx = 4096;
  const dim3 grid((unsigned)gx, (unsigned)(nbz > WIN_GRID_Y ? WIN_GRID_Y : nbz)), block(256);
  (void)hipGetLastError();
#define WIN_ACC(KT)                                                                                                                  \
  hipLaunchKernelGGL(window_accumulate_kernel<KT>, grid, block, 0, stream, pred, acc, nz, ny, nx, jobs, lo[0], lo[1], gx0, nbz, nby, \
                     ngx, H, W, K, R0, R1, R2, scale)
  switch (K) {
    case 1: WIN_ACC(1); break;
    case 2: WIN_ACC(2); break;
    case 3: WIN_ACC(3); break;
    case 4: WIN_ACC(4); break;
    default: WIN_ACC(0); break;
  }
#undef WIN_ACC
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- occupancy -------------------------------------------------------------------------------------------------------------------
// counts[(iz n1 + iy) n2 + ix] = the voxels with mask > 0 inside window (iz,iy,ix), clipped to the volume.  blockIdx.y is the window,
// blockIdx.x a run of its rows; a wave takes whole rows, counts in a register and a workgroup adds one integer to the window's count:
// integer sums commute, the counts are exact.  The starts are read from device memory and every coordinate is tested against the volume.
#define OCC_ROWS 16
__global__ __launch_bounds__(256) void window_occupancy_kernel(const float* __restrict__ mask, const int* __restrict__ starts, int* counts,
                                                               int n0, int n1, int n2, int D, int H, int W, int R0, int R1, int R2) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const int nwin = n0 * n1 * n2;
  for (int win = blockIdx.y; win < nwin; win += gridDim.y) {
    const int ix = win % n2, iy = (win / n2) % n1, iz = win / (n2 * n1);
    const int z0 = starts[iz], y0 = starts[n0 + iy], x0 = starts[n0 + n1 + ix];
    const long rows = (long)R0 * R1;
    int cnt = 0;
    const int lane = threadIdx.x & 63;
    for (long row = (long)blockIdx.x * OCC_ROWS + (threadIdx.x >> 6); row < rows && row < ((long)blockIdx.x + 1) * OCC_ROWS; row += 4) {
      const int d = (int)(row / R1), h = (int)(row - (long)d * R1);
      const int z = z0 + d, y = y0 + h;
      if (z < 0 || z >= D || y < 0 || y >= H) continue;
      const float* mrow = mask + ((long)z * H + y) * W;
      for (int w = lane; w < R2; w += 64) {
        const int xx = x0 + w;
        if (xx >= 0 && xx < W && mrow[xx] > 0.f) ++cnt;
      }
    }
    if (cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
      if (total) atomicAdd(&counts[win], total);
      total = 0;
    }
    __syncthreads();
  }
}

extern "C" int bts_window_occupancy(const float* mask, const int* starts, int* counts, int n0, int n1, int n2, int D, int H, int W, int R0,
                                    int R1, int R2, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || R0 <= 0 || R1 <= 0 || R2 <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0) return BTS_ERR_SHAPE;
  if ((long)n0 * n1 * n2 > 0x3fffffffL || (long)R0 * R1 * R2 > 0x7fffffffL || !win_fits(D, H, W, 1, R0, R1, R2)) return BTS_ERR_SHAPE;
  const int nwin = n0 * n1 * n2;
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)nwin * sizeof(int), stream);
  if (e != hipSuccess) return (int)e;
  const long gx = ((long)R0 * R1 + OCC_ROWS - 1) / OCC_ROWS;
  if (gx > 0x7fffffffL) return BTS_ERR_SHAPE;
  const dim3 grid((unsigned)gx, (unsigned)(nwin > WIN_GRID_Y ? WIN_GRID_Y : nwin)), block(256);
  (void)hipGetLastError();
  hipLaunchKernelGGL(window_occupancy_kernel, grid, block, 0, stream, mask, starts, counts, n0, n1, n2, D, H, W, R0, R1, R2);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
