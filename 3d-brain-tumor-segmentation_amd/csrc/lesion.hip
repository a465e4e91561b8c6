// What a lesion-wise score needs between the labelling (components.hip) and the distances (surface.hip); DESIGN section 21.
//   dilate3d         binary dilation of one region of a uint8 label map with scipy's 6 / 18 / 26 structuring element, iterated
//   lesion_pairs     one pass over (components of the dilated truth, truth, components of the prediction): the truth voxels per dilated
//                    component, and a hash table of the distinct (dilated component, predicted component) pairs with two counts each
//   component_boxes  the half-open bounding box of each component of a sorted list of roots
//   lesion_crop      two dense 0/1 maps of a box: the truth inside one dilated component, and the predicted components of a list
// Dense tensors, W innermost.  Plain HIP C++: vector loads and stores, integer atomics only, no inline assembly.  Every loop count is a
// function of the shape or of the table's capacity, no thread waits for a value another thread has yet to write, and every result is the
// same bytes in every run (the hash table's slot order is not, the sorted rows the caller makes of it are).
#include "common.h"
#include "bts_internal.h"

#include <limits.h>

#define LES_MAXK 8
#define DIL_SIDE 16                          // tile rows along H and along D, halo included: one row (a 64-bit word of W) per thread
#define DIL_ROWS (DIL_SIDE * DIL_SIDE)
#define DIL_BATCH 16                         // rows a wave loads before it looks at any of them
#define DIL_MAXFUSE 6                        // iterations of one pass: the halo on every side of the 64 x 16 x 16 tile
#define DIL_DEFAULT_FUSE 3
#define DIL_MAXITER 4096
#define LP_CHUNK 16                          // consecutive voxels per lane in the pairing pass, as in the sizes kernel
#define LP_MAXPROBE 4096
#define LES_BLOCKS 2048                      // grid cap of the streaming kernels: 8 workgroups per CU

#define LES_RLX_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ unsigned les_in_region(unsigned lab, unsigned top, unsigned class_mask) {
  return (class_mask >> (lab < top ? lab : top)) & 1u;
}

static bool les_region_ok(int K, int class_mask) { return K >= 2 && K <= LES_MAXK && class_mask >= 0 && class_mask < (1 << K); }

// ---- binary dilation ------------------------------------------------------------------------------------------------------------
// A row of the tile is one 64-bit word, bit b = the voxel at x0 + b (a ballot of a 64-byte load, as in the labelling), and a thread owns
// the row (ly, lz) of a 16 x 16 grid of rows in LDS.  One iteration: with hx(w) = w | w << 1 | w >> 1, `face` the OR of the four rows
// beside the own (dy or dz = +-1) and `diag` that of the four diagonal rows,
//   6 neighbours: hx(c) | face      18: hx(c | face) | diag      26: hx(c | face | diag)
// and the bits and rows outside the volume stay 0 (border_value = 0).  A pass runs f iterations on the tile; each one spoils one more
// ring of rows and of bits at the tile's edge (their neighbours are missing), so the inner 64 - 2 f bits of the inner 16 - 2 f rows are
// stored.  f = 0 stores the region itself.
__device__ __forceinline__ unsigned long long dil_hx(unsigned long long w) { return w | (w << 1) | (w >> 1); }

__global__ __launch_bounds__(256) void dilate_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int D, int H, int W,
                                                     int ntx, int nty, unsigned top, unsigned class_mask, int maxd, int f) {
  __shared__ unsigned long long row[2][DIL_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ow = 64 - 2 * f, orows = DIL_SIDE - 2 * f;
  const int bx = blockIdx.x % ntx, byz = blockIdx.x / ntx;
  const int x0 = bx * ow - f, y0 = (byz % nty) * orows - f, z0 = (byz / nty) * orows - f;
  const long HW = (long)H * W;
  const int x = x0 + lane;
  const bool xin = x >= 0 && x < W;
#pragma unroll 1
  for (int k0 = 0; k0 < DIL_ROWS / 4; k0 += DIL_BATCH) {   // a wave's 64 rows in batches: DIL_BATCH loads in flight, then their ballots
    unsigned set = 0u;
#pragma unroll
    for (int j = 0; j < DIL_BATCH; ++j) {
      const int r = wv + 4 * (k0 + j);
      const int y = y0 + (r & (DIL_SIDE - 1)), z = z0 + (r >> 4);
      if (xin && y >= 0 && y < H && z >= 0 && z < D) set |= les_in_region(in[z * HW + (long)y * W + x], top, class_mask) << j;
    }
#pragma unroll
    for (int j = 0; j < DIL_BATCH; ++j) {          // every lane of the wave takes part in the ballot
      const unsigned long long m = __ballot((set >> j) & 1u);
      if (lane == 0) row[0][wv + 4 * (k0 + j)] = m;
    }
  }
  __syncthreads();
  int cur = 0;
  if (f > 0) {
    const int t = threadIdx.x, ly = t & (DIL_SIDE - 1), lz = t >> 4;
    const bool rowin = y0 + ly >= 0 && y0 + ly < H && z0 + lz >= 0 && z0 + lz < D;
    const int lo = x0 < 0 ? -x0 : 0, hi = W - x0 < 64 ? W - x0 : 64;                 // 0 <= lo <= f < hi: the tile starts inside the volume
    const unsigned long long xmask = (hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
    const bool ym = ly > 0, yp = ly < DIL_SIDE - 1, zm = lz > 0, zp = lz < DIL_SIDE - 1;
    for (int it = 0; it < f; ++it) {
      const unsigned long long* a = row[cur];
      unsigned long long o = a[t];
      o |= (ym ? a[t - 1] : 0ull) | (yp ? a[t + 1] : 0ull) | (zm ? a[t - DIL_SIDE] : 0ull) | (zp ? a[t + DIL_SIDE] : 0ull);
      if (maxd == 1) {
        o |= dil_hx(a[t]);
      } else {
        const unsigned long long diag = (ym && zm ? a[t - DIL_SIDE - 1] : 0ull) | (yp && zm ? a[t - DIL_SIDE + 1] : 0ull) |
                                        (ym && zp ? a[t + DIL_SIDE - 1] : 0ull) | (yp && zp ? a[t + DIL_SIDE + 1] : 0ull);
        o = maxd == 2 ? (dil_hx(o) | diag) : dil_hx(o | diag);
      }
      row[cur ^ 1][t] = rowin ? (o & xmask) : 0ull;
      __syncthreads();
      cur ^= 1;
    }
  }
  if (lane < f || lane >= 64 - f || x >= W) return;                                  // x >= 0 here: lane >= f
#pragma unroll 4
  for (int k = 0; k < DIL_ROWS / 4; ++k) {
    const int r = wv + 4 * k;
    const int ly = r & (DIL_SIDE - 1), lz = r >> 4;
    const int y = y0 + ly, z = z0 + lz;
    if (ly < f || ly >= DIL_SIDE - f || lz < f || lz >= DIL_SIDE - f || y >= H || z >= D) continue;
    out[z * HW + (long)y * W + x] = (uint8_t)((row[cur][r] >> lane) & 1ull);
  }
}

static int dil_fuse(int iterations, int fuse) {
  const int f = fuse > 0 ? fuse : DIL_DEFAULT_FUSE;
  return f < iterations ? f : iterations;
}

static bool dil_args_ok(int D, int H, int W, int iterations, int fuse) {
  if (D <= 0 || H <= 0 || W <= 0 || iterations < 0 || iterations > DIL_MAXITER || fuse < 0 || fuse > DIL_MAXFUSE) return false;
  const long lim = 0x7fffffffL, dh = (long)D * H;
  return dh < lim && dh * W < lim;                                                  // fewer than 2^31 tiles at every f
}

extern "C" long bts_dilate3d_workspace(int D, int H, int W, int iterations, int fuse) {
  if (!dil_args_ok(D, H, W, iterations, fuse)) return BTS_ERR_SHAPE;
  const int f = dil_fuse(iterations, fuse);
  const int passes = f ? (iterations + f - 1) / f : 1;
  return passes >= 2 ? (long)D * H * W : 0;
}

extern "C" int bts_dilate3d(const uint8_t* lab, uint8_t* out, int D, int H, int W, int K, int class_mask, int connectivity,
                            int iterations, int fuse, void* work, hipStream_t stream) {
  if (!dil_args_ok(D, H, W, iterations, fuse) || !les_region_ok(K, class_mask)) return BTS_ERR_SHAPE;
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) return BTS_ERR_SHAPE;
  const int f = dil_fuse(iterations, fuse);
  const int passes = f ? (iterations + f - 1) / f : 1;
  if (passes >= 2 && work == nullptr) return BTS_ERR_WORKSPACE;
  const int maxd = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
  const uint8_t* src = lab;
  unsigned top = (unsigned)K - 1u, mask = (unsigned)class_mask;
  int left = iterations;
  (void)hipGetLastError();
  for (int p = 0; p < passes; ++p) {
    const int fp = left < f ? left : f;
    uint8_t* dst = ((passes - 1 - p) & 1) ? static_cast<uint8_t*>(work) : out;      // the last pass writes `out`
    const int ow = 64 - 2 * fp, orows = DIL_SIDE - 2 * fp;
    const int ntx = (W + ow - 1) / ow, nty = (H + orows - 1) / orows, ntz = (D + orows - 1) / orows;
    hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)((long)ntx * nty * ntz)), dim3(256), 0, stream, src, dst, D, H, W, ntx, nty, top, mask,
                       maxd, fp);
    BTS_LAUNCH_CHECK();
    src = dst;
    top = 1u;                                                                       // the passes after the first read a 0/1 map
    mask = 2u;
    left -= fp;
  }
  return BTS_OK;
}

// ---- lesion / component pairing ---------------------------------------------------------------------------------------------------
// table: `capacity` 64-bit keys, then `capacity` pairs of int32 counts (reach, overlap).  key = (td << 32) | pc with td, pc the values of
// the two component maps (root + 1, so a key is never 0 = empty).  Open addressing, linear probing of at most min(capacity, 4096)
// slots; a slot is claimed by one 64-bit compare-and-swap and never freed, so every attempt for a key walks the same occupied slots:
// either all of them end at the key's slot or all of them fail, and a stored pair holds its complete counts also when others found no
// room.  status[0] = pairs stored, status[1] = attempts (runs of equal pairs in a lane's voxels) that found no room: an upper bound of
// the pairs that are missing.  Integer sums commute: the counts are exact in every run.
__device__ __forceinline__ unsigned long long lp_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  return k ^ (k >> 33);
}

__device__ void lp_add(unsigned long long* keys, int* counts, long cap, int probes, unsigned long long* status, unsigned long long key,
                       int reach, int overlap) {
  long slot = (long)(lp_hash(key) % (unsigned long long)cap);
  for (int p = 0; p < probes; ++p) {
    unsigned long long cur = LES_RLX_AGENT(&keys[slot]);
    if (cur == 0ull) {
      cur = atomicCAS(&keys[slot], 0ull, key);
      if (cur == 0ull) {
        atomicAdd(&status[0], 1ull);
        cur = key;
      }
    }
    if (cur == key) {
      atomicAdd(&counts[2 * slot], reach);
      if (overlap) atomicAdd(&counts[2 * slot + 1], overlap);
      return;
    }
    if (++slot == cap) slot = 0;
  }
  atomicAdd(&status[1], 1ull);
}

__global__ __launch_bounds__(256) void lesion_pairs_kernel(const int* __restrict__ td, const uint8_t* __restrict__ truth,
                                                           const int* __restrict__ pc, long n, int vec, unsigned top, unsigned class_mask,
                                                           int* lesion_vox, unsigned long long* keys, int* counts, long cap, int probes,
                                                           unsigned long long* status) {
  {
    const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * LP_CHUNK;
    if (e0 >= n) return;
    const int m = n - e0 < LP_CHUNK ? (int)(n - e0) : LP_CHUNK;
    int a[LP_CHUNK], b[LP_CHUNK];
    unsigned any = 0u;
    if (vec && m == LP_CHUNK) {
#pragma unroll
      for (int j = 0; j < LP_CHUNK / 4; ++j) {
        const int4 t = *reinterpret_cast<const int4*>(td + e0 + 4 * j);
        a[4 * j] = t.x; a[4 * j + 1] = t.y; a[4 * j + 2] = t.z; a[4 * j + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < LP_CHUNK; ++j) a[j] = j < m ? td[e0 + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < LP_CHUNK; ++j) {
      if (a[j] < 0 || (long)a[j] > n) a[j] = 0;                                      // not a value components3d writes: no index from it
      any |= (unsigned)a[j];
    }
    if (!any) return;                                                                // outside every dilated lesion: most of a scan
    if (vec && m == LP_CHUNK) {
#pragma unroll
      for (int j = 0; j < LP_CHUNK / 4; ++j) {
        const int4 t = *reinterpret_cast<const int4*>(pc + e0 + 4 * j);
        b[4 * j] = t.x; b[4 * j + 1] = t.y; b[4 * j + 2] = t.z; b[4 * j + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < LP_CHUNK; ++j) b[j] = j < m ? pc[e0 + j] : 0;
    }
    int cura = 0, cnt = 0, pa = 0, pb = 0, reach = 0, ov = 0;
#pragma unroll
    for (int j = 0; j <= LP_CHUNK; ++j) {                                            // j == LP_CHUNK: the flush
      const int aj = j < LP_CHUNK ? a[j] : 0;
      const int bj = (j < LP_CHUNK && aj != 0 && b[j] > 0) ? b[j] : 0;
      const int tj = (j < m && aj != 0) ? (int)les_in_region(truth[e0 + j], top, class_mask) : 0;
      if (aj != cura) {
        if (cura != 0 && cnt != 0) atomicAdd(&lesion_vox[cura - 1], cnt);
        cura = aj;
        cnt = 0;
      }
      cnt += tj;
      const bool has = bj != 0;
      if (!(has && aj == pa && bj == pb)) {
        if (pa != 0)
          lp_add(keys, counts, cap, probes, status, ((unsigned long long)(unsigned)pa << 32) | (unsigned long long)(unsigned)pb, reach, ov);
        pa = has ? aj : 0;
        pb = bj;
        reach = 0;
        ov = 0;
      }
      if (has) {
        ++reach;
        ov += tj;
      }
    }
  }
}

extern "C" long bts_lesion_pairs_table_bytes(long capacity) {
  if (capacity < 1 || capacity > (1L << 32)) return BTS_ERR_SHAPE;
  return capacity * 16;
}

extern "C" int bts_lesion_pairs(const int* td_comp, const uint8_t* truth, const int* pred_comp, long n, int K, int class_mask,
                                int* lesion_vox, void* table, long capacity, long* status, hipStream_t stream) {
  if (n < 0 || n >= 0x7fffffffL || !les_region_ok(K, class_mask) || capacity < 1 || capacity > (1L << 32)) return BTS_ERR_SHAPE;
  hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(long), stream);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(table, 0, (size_t)capacity * 16, stream);
  if (e != hipSuccess) return (int)e;
  if (n == 0) return BTS_OK;
  e = hipMemsetAsync(lesion_vox, 0, (size_t)n * sizeof(int), stream);
  if (e != hipSuccess) return (int)e;
  const long per = 256L * LP_CHUNK;
  const long blocks = (n + per - 1) / per;
  const int vec = ((reinterpret_cast<uintptr_t>(td_comp) | reinterpret_cast<uintptr_t>(pred_comp)) & 15) == 0;
  unsigned long long* keys = static_cast<unsigned long long*>(table);
  (void)hipGetLastError();
  hipLaunchKernelGGL(lesion_pairs_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, td_comp, truth, pred_comp, n, vec, (unsigned)K - 1u,
                     (unsigned)class_mask, lesion_vox, keys, reinterpret_cast<int*>(keys + capacity), capacity,
                     (int)(capacity < LP_MAXPROBE ? capacity : LP_MAXPROBE), reinterpret_cast<unsigned long long*>(status));
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- bounding boxes ------------------------------------------------------------------------------------------------------------------
// index of root r in the ascending list, -1 when it is not there; the interval halves every turn
__device__ __forceinline__ int les_find(const int* __restrict__ roots, int m, int r) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (roots[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return (lo < m && roots[lo] == r) ? lo : -1;
}

__global__ __launch_bounds__(256) void boxes_init_kernel(int* box, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) box[i] = (i % 6) < 3 ? INT_MAX : 0;
}

// A minimum and a maximum do not depend on the order they are taken in.  A wave owns 64 consecutive voxels; per component among them
// (mostly one) the six extremes are reduced across the lanes and ONE lane reads the box and issues an atomic only where the wave's
// extreme lies outside it: a large component costs a few atomics per wave that sees a stale box, not six per voxel.  The loops are
// wave-uniform (the first index and the ballots are), and every turn of the inner one retires its leader's component.
__global__ __launch_bounds__(256) void boxes_kernel(const int* __restrict__ comp, int H, int W, long n, const int* __restrict__ roots, int m,
                                                    int* box) {
  const long HW = (long)H * W;
  const int lane = threadIdx.x & 63;
  for (long v0 = (long)blockIdx.x * 256 + (threadIdx.x & ~63); v0 < n; v0 += (long)gridDim.x * 256) {
    const long v = v0 + lane;
    int i = -1, d = 0, h = 0, w = 0;
    if (v < n) {
      const int c = comp[v];
      if (c > 0) i = les_find(roots, m, c - 1);
      if (i >= 0) {
        d = (int)(v / HW);
        const long r = v - d * HW;
        h = (int)(r / W);
        w = (int)(r - (long)h * W);
      }
    }
    unsigned long long todo = __ballot(i >= 0);
    while (todo) {
      const int leader = __builtin_ctzll(todo);
      const bool mine = i == __shfl(i, leader, 64);
      int lo0 = mine ? d : INT_MAX, lo1 = mine ? h : INT_MAX, lo2 = mine ? w : INT_MAX;
      int hi0 = mine ? d + 1 : 0, hi1 = mine ? h + 1 : 0, hi2 = mine ? w + 1 : 0;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        lo0 = min(lo0, __shfl_xor(lo0, s, 64));
        lo1 = min(lo1, __shfl_xor(lo1, s, 64));
        lo2 = min(lo2, __shfl_xor(lo2, s, 64));
        hi0 = max(hi0, __shfl_xor(hi0, s, 64));
        hi1 = max(hi1, __shfl_xor(hi1, s, 64));
        hi2 = max(hi2, __shfl_xor(hi2, s, 64));
      }
      if (lane == leader) {
        int* b = box + 6 * i;
        if (lo0 < LES_RLX_AGENT(&b[0])) atomicMin(&b[0], lo0);
        if (lo1 < LES_RLX_AGENT(&b[1])) atomicMin(&b[1], lo1);
        if (lo2 < LES_RLX_AGENT(&b[2])) atomicMin(&b[2], lo2);
        if (hi0 > LES_RLX_AGENT(&b[3])) atomicMax(&b[3], hi0);
        if (hi1 > LES_RLX_AGENT(&b[4])) atomicMax(&b[4], hi1);
        if (hi2 > LES_RLX_AGENT(&b[5])) atomicMax(&b[5], hi2);
      }
      todo &= ~__ballot(mine);
    }
  }
}

extern "C" int bts_component_boxes(const int* comp, int D, int H, int W, const int* roots, int nroots, int* boxes, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || nroots < 0 || nroots > (1 << 28)) return BTS_ERR_SHAPE;
  const long lim = 0x7fffffffL, dh = (long)D * H;
  if (dh >= lim || dh * W >= lim) return BTS_ERR_SHAPE;
  if (nroots == 0) return BTS_OK;
  const long n = dh * W;
  (void)hipGetLastError();
  hipLaunchKernelGGL(boxes_init_kernel, dim3((unsigned)((6L * nroots + 255) / 256)), dim3(256), 0, stream, boxes, 6 * nroots);
  BTS_LAUNCH_CHECK();
  long blocks = (n + 255) / 256;
  blocks = blocks > LES_BLOCKS ? LES_BLOCKS : blocks;
  hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, comp, H, W, n, roots, nroots, boxes);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- lesion crop ---------------------------------------------------------------------------------------------------------------------
// An item is four consecutive voxels of the flat box: one 4-byte store per map where both are 4-byte aligned (VEC), byte by byte
// otherwise and in the tail.
struct LesBox {
  int d0, h0, w0, bd, bh, bw;
};

template <bool VEC>
__global__ __launch_bounds__(256) void lesion_crop_kernel(const int* __restrict__ td, const uint8_t* __restrict__ truth,
                                                          const int* __restrict__ pc, int H, int W, LesBox bx, long nbox, long nitems,
                                                          unsigned top, unsigned class_mask, int td_value, const int* __restrict__ roots,
                                                          int nroots, uint8_t* __restrict__ g, uint8_t* __restrict__ mm) {
  const long HW = (long)H * W, bhw = (long)bx.bh * bx.bw;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < nitems; it += (long)gridDim.x * 256) {
    const long v0 = it * 4;
    const int n = nbox - v0 < 4 ? (int)(nbox - v0) : 4;
    int d = (int)(v0 / bhw);
    const long r = v0 - d * bhw;
    int h = (int)(r / bx.bw), w = (int)(r - (long)h * bx.bw);
    unsigned gw = 0u, mw = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        const long src = (bx.d0 + d) * HW + (long)(bx.h0 + h) * W + bx.w0 + w;
        if (td[src] == td_value && les_in_region(truth[src], top, class_mask)) gw |= 1u << (8 * k);
        const int c = pc[src];
        if (c > 0 && les_find(roots, nroots, c - 1) >= 0) mw |= 1u << (8 * k);
        if (++w == bx.bw) {
          w = 0;
          if (++h == bx.bh) { h = 0; ++d; }
        }
      }
    }
    if (VEC && n == 4) {
      *reinterpret_cast<unsigned*>(g + v0) = gw;
      *reinterpret_cast<unsigned*>(mm + v0) = mw;
    } else {
      for (int k = 0; k < n; ++k) {
        g[v0 + k] = (uint8_t)((gw >> (8 * k)) & 255u);
        mm[v0 + k] = (uint8_t)((mw >> (8 * k)) & 255u);
      }
    }
  }
}

extern "C" int bts_lesion_crop(const int* td_comp, const uint8_t* truth, const int* pred_comp, int D, int H, int W, int K, int class_mask,
                               int d0, int h0, int w0, int d1, int h1, int w1, int td_root, const int* roots, int nroots, uint8_t* g,
                               uint8_t* m, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || !les_region_ok(K, class_mask) || nroots < 0 || nroots > (1 << 28)) return BTS_ERR_SHAPE;
  const long lim = 0x7fffffffL, dh = (long)D * H;
  if (dh >= lim || dh * W >= lim) return BTS_ERR_SHAPE;
  if (d0 < 0 || h0 < 0 || w0 < 0 || d1 > D || h1 > H || w1 > W || d0 >= d1 || h0 >= h1 || w0 >= w1) return BTS_ERR_SHAPE;
  if (td_root < 0 || td_root >= dh * W) return BTS_ERR_SHAPE;
  LesBox bx = {d0, h0, w0, d1 - d0, h1 - h0, w1 - w0};
  const long nbox = (long)bx.bd * bx.bh * bx.bw, nitems = (nbox + 3) / 4;
  long blocks = (nitems + 255) / 256;
  blocks = blocks > LES_BLOCKS ? LES_BLOCKS : blocks;
  const bool vec = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m)) & 3) == 0;
  (void)hipGetLastError();
  if (vec) hipLaunchKernelGGL(lesion_crop_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, td_comp, truth, pred_comp, H, W, bx, nbox,
                              nitems, (unsigned)K - 1u, (unsigned)class_mask, td_root + 1, roots, nroots, g, m);
  else hipLaunchKernelGGL(lesion_crop_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, td_comp, truth, pred_comp, H, W, bx, nbox,
                          nitems, (unsigned)K - 1u, (unsigned)class_mask, td_root + 1, roots, nroots, g, m);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
