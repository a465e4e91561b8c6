// Class-location tables for foreground-oversampled training crops (the nnU-Net / batchgenerators recipe: a share of the patches is centred
// on a random voxel of a random foreground class, taken from a per-case table built once).  No reference counterpart: train.py:26 crops
// uniformly.
//   bts_class_locations   label volume (V floats, label k in 1..out_ch = class k-1, the convention of augment.hip's one-hot)
//                         -> counts[c] = n_c, the voxels whose label is exactly c+1, and loc[c][0..K): the linear indices of the class's
//                         voxels of rank 0, s_c, 2 s_c, ... in ascending index order, s_c = max(1, ceil(n_c / K)), the rest -1.
// The table is a pure function of the volume: a voxel's slot follows from its RANK among the voxels of its class, never from the order in
// which waves arrive (no atomic cursor).  Three launches over a fixed partition of the volume: a workgroup of four waves takes SAMP_CHUNK
// = 4096 consecutive voxels, each wave SAMP_UNIT = 1024 of them in four steps of 256 (a lane loads four neighbours as one 16-byte access):
//   1. count     one __ballot per class and voxel-of-the-lane, __popcll, the four waves' sums added through LDS -> cnt[c][workgroup]
//   2. scan      one workgroup per class: exclusive prefix of cnt[c][.] in place (the rank of each chunk's first voxel of the class),
//                n_c -> counts, and s_c, m_c = ceil(n_c / s_c) for the third launch
//   3. scatter   the walk of launch 1 again; rank = chunk base + the counts of the waves before + the wave's running count +
//                __popcll(ballots & lanes below) + the lane's own earlier voxels; a voxel whose rank is a multiple of s_c is stored at
//                loc[c][rank / s_c].  The same launch writes -1 to the entries m_c..K-1, which no voxel owns.
// Integer arithmetic only (the label test is an exact float compare), plain vector stores, every one of the out_ch * K entries written
// exactly once per call.  Two reads of the 4 V bytes; the stores are at most out_ch * K ints.
#include "common.h"
#include "bts_internal.h"

#define SAMP_MAXC 8
#define SAMP_STEP 256                      // voxels a wave takes per step: 64 lanes x 4
#define SAMP_STEPS 4
#define SAMP_UNIT (SAMP_STEP * SAMP_STEPS) // voxels of one wave
#define SAMP_WAVES 4
#define SAMP_CHUNK (SAMP_UNIT * SAMP_WAVES) // voxels of one workgroup

// The 16 labels a lane owns: voxels first + 256 s + 4 lane + e, s < 4 steps, e < 4; a voxel at or past V reads as 0 (in no class).
// A 16-byte access where y is 16-byte aligned and the four voxels exist, else voxel by voxel.
__device__ __forceinline__ void samp_load(const float* __restrict__ y, long first, int lane, long V, float (&v)[SAMP_STEPS][4]) {
  const bool vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
#pragma unroll
  for (int s = 0; s < SAMP_STEPS; ++s) {
    const long i = first + s * SAMP_STEP + 4 * lane;
    if (vec && i + 4 <= V) {
      const float4 t = *reinterpret_cast<const float4*>(y + i);
      v[s][0] = t.x; v[s][1] = t.y; v[s][2] = t.z; v[s][3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[s][e] = (i + e < V) ? y[i + e] : 0.f;
    }
  }
}
// the wave's voxels that carry `label` (all 64 lanes call it together)
__device__ __forceinline__ int samp_wave_count(const float (&v)[SAMP_STEPS][4], float label) {
  int n = 0;
#pragma unroll
  for (int s = 0; s < SAMP_STEPS; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) n += __popcll(__ballot(v[s][e] == label));
  return n;
}

__global__ __launch_bounds__(64 * SAMP_WAVES) void samp_count_kernel(const float* __restrict__ y, int* __restrict__ cnt, long V, int out_ch) {
  __shared__ int wcnt[SAMP_WAVES][SAMP_MAXC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float v[SAMP_STEPS][4];
  samp_load(y, (long)blockIdx.x * SAMP_CHUNK + wave * SAMP_UNIT, lane, V, v);
#pragma unroll
  for (int c = 0; c < SAMP_MAXC; ++c) {
    if (c < out_ch) {
      const int n = samp_wave_count(v, (float)(c + 1));
      if (lane == 0) wcnt[wave][c] = n;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < out_ch) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < SAMP_WAVES; ++w) n += wcnt[w][threadIdx.x];
    cnt[(long)threadIdx.x * gridDim.x + blockIdx.x] = n;
  }
}

// One workgroup of 256 per class.  A thread owns a run of consecutive chunks: it sums them, the 256 sums are scanned by the first wave
// (four per lane, __shfl_up across the lanes), and the thread rewrites its run as exclusive prefixes.  par: s_c at [c], m_c at
// [SAMP_MAXC + c].
__global__ __launch_bounds__(256) void samp_scan_kernel(int* __restrict__ cnt, int* __restrict__ par, long* __restrict__ counts, int chunks,
                                                        int K) {
  __shared__ int sh[256];
  const int c = blockIdx.x, t = threadIdx.x;
  int* row = cnt + (long)c * chunks;
  const int per = (chunks + 255) / 256;
  const int a = min(t * per, chunks), b = min(a + per, chunks);
  int sum = 0;
  for (int u = a; u < b; ++u) sum += row[u];
  sh[t] = sum;
  __syncthreads();
  if (t < 64) {
    const int a0 = sh[4 * t], a1 = sh[4 * t + 1], a2 = sh[4 * t + 2], a3 = sh[4 * t + 3];
    const int own = (a0 + a1) + (a2 + a3);
    int inc = own;                                         // inclusive prefix over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_up(inc, o, 64);
      if (t >= o) inc += x;
    }
    const int ex = inc - own;
    sh[4 * t] = ex; sh[4 * t + 1] = ex + a0; sh[4 * t + 2] = ex + a0 + a1; sh[4 * t + 3] = ex + a0 + a1 + a2;
    if (t == 63) {
      const int n = inc;                                   // n_c <= V < 2^31
      const int s = n <= K ? 1 : (int)(((long)n + K - 1) / K);
      counts[c] = n;
      par[c] = s;
      par[SAMP_MAXC + c] = (n + s - 1) / s;                // m_c <= K
    }
  }
  __syncthreads();
  int run = sh[t];
  for (int u = a; u < b; ++u) { const int x = row[u]; row[u] = run; run += x; }
}

__global__ __launch_bounds__(64 * SAMP_WAVES) void samp_scatter_kernel(const float* __restrict__ y, const int* __restrict__ base,
                                                                       const int* __restrict__ par, int* __restrict__ loc, long V,
                                                                       int out_ch, int K) {
  __shared__ int wcnt[SAMP_WAVES][SAMP_MAXC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // ---- the entries no voxel owns: m_c .. K-1 of every class ----
  const long nthreads = (long)gridDim.x * blockDim.x;
  for (int c = 0; c < out_ch; ++c)
    for (long j = par[SAMP_MAXC + c] + (long)blockIdx.x * blockDim.x + threadIdx.x; j < K; j += nthreads) loc[(long)c * K + j] = -1;
  const long first = (long)blockIdx.x * SAMP_CHUNK + wave * SAMP_UNIT;
  const unsigned long long below = (1ull << lane) - 1ull;
  float v[SAMP_STEPS][4];
  samp_load(y, first, lane, V, v);
#pragma unroll
  for (int c = 0; c < SAMP_MAXC; ++c) {
    if (c < out_ch) {
      const int n = samp_wave_count(v, (float)(c + 1));
      if (lane == 0) wcnt[wave][c] = n;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < SAMP_MAXC; ++c) {
    if (c < out_ch) {
      const float label = (float)(c + 1);
      const int stride = par[c];
      int* row = loc + (long)c * K;
      int run = base[(long)c * gridDim.x + blockIdx.x];    // rank of the first voxel of class c in this step of this wave
      for (int w = 0; w < wave; ++w) run += wcnt[w][c];
#pragma unroll
      for (int s = 0; s < SAMP_STEPS; ++s) {
        int before = 0, total = 0;                         // ... of the class in the lanes below, in the whole step
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned long long m = __ballot(v[s][e] == label);
          before += __popcll(m & below);
          total += __popcll(m);
        }
        int rank = run + before;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (v[s][e] == label) {
            const int idx = (int)(first + s * SAMP_STEP + 4 * lane + e);
            if (stride == 1) row[rank] = idx;
            else if (rank % stride == 0) row[rank / stride] = idx;
            ++rank;
          }
        }
        run += total;
      }
    }
  }
}

static long samp_chunks(long V) { return (V + SAMP_CHUNK - 1) / SAMP_CHUNK; }      // < 2^19
static bool samp_shape_ok(long V, int out_ch) { return V >= 1 && V < (1l << 31) && out_ch >= 1 && out_ch <= SAMP_MAXC; }

extern "C" long bts_class_locations_workspace(long V, int out_ch) {
  if (!samp_shape_ok(V, out_ch)) return BTS_ERR_SHAPE;
  return ((long)out_ch * samp_chunks(V) + 2 * SAMP_MAXC) * (long)sizeof(int);
}

extern "C" int bts_class_locations(const float* y, long* counts, int* loc, void* workspace, long workspace_bytes, long V, int out_ch,
                                   int K, hipStream_t stream) {
  if (!samp_shape_ok(V, out_ch) || K < 1 || y == nullptr || counts == nullptr || loc == nullptr) return BTS_ERR_SHAPE;
  if (workspace == nullptr || workspace_bytes < bts_class_locations_workspace(V, out_ch)) return BTS_ERR_WORKSPACE;
  const int chunks = (int)samp_chunks(V);
  int* cnt = reinterpret_cast<int*>(workspace);
  int* par = cnt + (long)out_ch * chunks;
  (void)hipGetLastError(); hipLaunchKernelGGL(samp_count_kernel, dim3(chunks), dim3(64 * SAMP_WAVES), 0, stream, y, cnt, V, out_ch);
  BTS_LAUNCH_CHECK();
  (void)hipGetLastError(); hipLaunchKernelGGL(samp_scan_kernel, dim3(out_ch), dim3(256), 0, stream, cnt, par, counts, chunks, K);
  BTS_LAUNCH_CHECK();
  (void)hipGetLastError(); hipLaunchKernelGGL(samp_scatter_kernel, dim3(chunks), dim3(64 * SAMP_WAVES), 0, stream, y, cnt, par, loc, V, out_ch, K);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
