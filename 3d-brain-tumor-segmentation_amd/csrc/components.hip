// Connected components of one region of a uint8 label map, and what post-processing does with them.
//   components3d       comp (int32) = 1 + the smallest linear index of the voxel's component, 0 outside the region; 6 / 18 / 26 neighbours
//   component_sizes    size[root] = voxels of the component, and the number of components
//   component_largest  one 64-bit key (size << 32) | (0xFFFFFFFF - root): the largest component, the smallest root among equals
//   components_apply   in place: voxels of components that fail (size >= min_voxels [and root == the key's]) become `fill`
//   region_relabel     in place: a region of fewer than `limit` voxels (counted by bts_label_confusion) becomes `fill`
// Union-find with the parent of voxel v kept as comp[v] = parent + 1 from the first kernel to the last (0: not of the region), so a
// root is comp[v] == v + 1 and every later write of an ancestor keeps the map valid.  Parents only ever DECREASE and always name a
// voxel of the same component: a stale read is still an ancestor.  Across workgroups correctness rests on the return values of
// agent-scope integer atomics and on kernel boundaries alone: no fences, flags, tickets or epochs, and no thread waits for a value
// another thread has yet to write.  Every loop strictly decreases an index.  Plain HIP C++, no inline assembly.
#include "common.h"
#include "bts_internal.h"

#define CC_MAXK 8
#define CC_TW 64                       // tile: one wave along W, so a row's region bits are one ballot
#define CC_TH 8
#define CC_TD 8
#define CC_ROWS (CC_TH * CC_TD)        // 64 rows, 16 per wave
#define CC_TILE (CC_ROWS * CC_TW)      // 4096 voxels: 16 KiB of parents in LDS, 8 workgroups per CU
#define CC_CHUNK 16                    // consecutive elements per lane in the sizes kernel

#define CC_RLX_WG(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define CC_RLX_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ unsigned cc_in_region(unsigned lab, unsigned top, unsigned class_mask) {
  return (class_mask >> (lab < top ? lab : top)) & 1u;
}

// The backward half of the stencil by rows: the four rows (dz,dy) in front of a voxel's own, in order (0,-1) (-1,0) (-1,-1) (-1,+1).
// nd = |dz| + |dy|; the voxel straight across (dx = 0) is a neighbour when nd <= maxd, the two beside it (dx = -1, +1) when
// nd + 1 <= maxd; maxd = 1, 2, 3 for 6, 18, 26 neighbours.  (dx = -1 in the voxel's own row is the run / the x seam.)
__device__ __forceinline__ void cc_row(int k, int& dz, int& dy) {
  dz = k == 0 ? 0 : -1;
  dy = k == 0 ? -1 : (k == 1 ? 0 : (k == 2 ? -1 : 1));
}

// ---- local: a tile in LDS --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_lds_find(int* par, int a) {
  for (;;) {                                     // par[a] <= a: the index strictly decreases until a root
    const int p = CC_RLX_WG(&par[a]);
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void cc_lds_union(int* par, int a, int b) {
  for (;;) {                                     // a + b strictly decreases: finds only go down, and `old` below is < a
    a = cc_lds_find(par, a);
    b = cc_lds_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;                        // a was a root and now hangs under b
    a = old;                                     // a had moved already: its former parent and b are still to be joined
  }
}

__global__ __launch_bounds__(256) void cc_local_kernel(const uint8_t* __restrict__ lab, int* __restrict__ comp, int D, int H, int W,
                                                       int ntx, int nty, unsigned top, unsigned class_mask, int maxd) {
  __shared__ int par[CC_TILE];
  __shared__ unsigned long long rowmask[CC_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int bx = blockIdx.x % ntx, byz = blockIdx.x / ntx;
  const int x0 = bx * CC_TW, y0 = (byz % nty) * CC_TH, z0 = (byz / nty) * CC_TD;
  const int x = x0 + lane;
  const long HW = (long)H * W;
  unsigned mine = 0u;                            // bit k: my voxel of row wv + 4 k is of the region
  // 1. x-runs: the parent of a voxel is the start of its run in the row (every lane of the wave takes part in the ballot)
#pragma unroll
  for (int k = 0; k < CC_ROWS / 4; ++k) {
    const int r = wv + 4 * k;
    const int y = y0 + (r & (CC_TH - 1)), z = z0 + (r >> 3);
    bool in = false;
    if (x < W && y < H && z < D) in = cc_in_region(lab[z * HW + (long)y * W + x], top, class_mask) != 0u;
    const unsigned long long m = __ballot(in);
    if (lane == 0) rowmask[r] = m;
    int start = lane;
    if (in) {
      const unsigned long long gaps = ~m & ((1ull << lane) - 1ull);         // voxels outside the region before mine
      start = gaps ? 64 - __builtin_clzll(gaps) : 0;
      mine |= 1u << k;
    }
    par[r * CC_TW + lane] = r * CC_TW + start;
  }
  __syncthreads();
  // 2. rows and planes of the tile.  A union is left out where a neighbour's makes it redundant: straight across when the voxels to the
  // left of both are of the region (the left voxel joins the same two runs), beside when the voxel straight across is (same run).
#pragma unroll 1
  for (int k = 0; k < CC_ROWS / 4; ++k) {
    if (!((mine >> k) & 1u)) continue;
    const int r = wv + 4 * k;
    const int ly = r & (CC_TH - 1), lz = r >> 3;
    const bool left_me = lane > 0 && ((rowmask[r] >> (lane - 1)) & 1ull);
    for (int q = 0; q < 4; ++q) {
      int dz, dy;
      cc_row(q, dz, dy);
      const int nd = (dz ? 1 : 0) + (dy ? 1 : 0);
      if (nd > maxd) continue;
      const int ny = ly + dy, nz = lz + dz;
      if (ny < 0 || ny >= CC_TH || nz < 0) continue;                        // another tile: the seam kernel's
      const int nr = nz * CC_TH + ny;
      const unsigned long long nm = rowmask[nr];
      if ((nm >> lane) & 1ull) {
        if (!(left_me && ((nm >> (lane - 1)) & 1ull))) cc_lds_union(par, r * CC_TW + lane, nr * CC_TW + lane);
      } else if (nd + 1 <= maxd) {
        if (lane > 0 && ((nm >> (lane - 1)) & 1ull)) cc_lds_union(par, r * CC_TW + lane, nr * CC_TW + lane - 1);
        if (lane < CC_TW - 1 && ((nm >> (lane + 1)) & 1ull)) cc_lds_union(par, r * CC_TW + lane, nr * CC_TW + lane + 1);
      }
    }
  }
  __syncthreads();
  // 3. tile-local root -> global linear index (the local order is the global order inside a tile), + 1; 0 outside the region
#pragma unroll 1
  for (int k = 0; k < CC_ROWS / 4; ++k) {
    const int r = wv + 4 * k;
    const int y = y0 + (r & (CC_TH - 1)), z = z0 + (r >> 3);
    if (x >= W || y >= H || z >= D) continue;
    int c = 0;
    if ((mine >> k) & 1u) {
      const int root = cc_lds_find(par, r * CC_TW + lane);
      const int rr = root >> 6;
      c = (int)((z0 + (rr >> 3)) * HW + (long)(y0 + (rr & (CC_TH - 1))) * W + x0 + (root & (CC_TW - 1))) + 1;
    }
    comp[z * HW + (long)y * W + x] = c;
  }
}

// ---- seams: neighbours in different tiles ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_find(int* comp, int a) {
  for (;;) {                                     // comp[a] - 1 <= a: the index strictly decreases until a root
    const int p = CC_RLX_AGENT(&comp[a]) - 1;
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void cc_union(int* comp, int a, int b) {
  for (;;) {                                     // a + b strictly decreases: finds only go down, and `old` below is < a
    a = cc_find(comp, a);
    b = cc_find(comp, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&comp[a], b + 1) - 1;                         // agent scope: the returned value decides, nothing else
    if (old == a) return;                        // a was a root and now hangs under b
    a = old;                                     // a had moved already: its former parent and b are still to be joined
  }
}

// The tile grid of the local kernel, one wave per row again.  A voxel takes part when a neighbour of the backward half lies in another
// tile: it is on a face of its tile.  comp[u] != 0 is "u is of the region" (the local kernel wrote every element; zero never changes).
__global__ __launch_bounds__(256) void cc_seam_kernel(int* comp, int D, int H, int W, int ntx, int nty, int maxd) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int bx = blockIdx.x % ntx, byz = blockIdx.x / ntx;
  const int x0 = bx * CC_TW, y0 = (byz % nty) * CC_TH, z0 = (byz / nty) * CC_TD;
  const int x = x0 + lane;
  const long HW = (long)H * W;
  if (x >= W) return;
#pragma unroll 1
  for (int k = 0; k < CC_ROWS / 4; ++k) {
    const int r = wv + 4 * k;
    const int ly = r & (CC_TH - 1), lz = r >> 3;
    const int y = y0 + ly, z = z0 + lz;
    if (y >= H || z >= D) continue;
    const bool face = ly == 0 || ly == CC_TH - 1 || lz == 0;
    if (!face && lane != 0 && lane != CC_TW - 1) continue;
    const long v = z * HW + (long)y * W + x;
    if (CC_RLX_AGENT(&comp[v]) == 0) continue;
    const bool left = x > 0 && CC_RLX_AGENT(&comp[v - 1]) != 0;
    if (left && lane == 0) cc_union(comp, (int)v, (int)v - 1);              // the run goes on in the tile to the left
    for (int q = 0; q < 4; ++q) {
      int dz, dy;
      cc_row(q, dz, dy);
      const int nd = (dz ? 1 : 0) + (dy ? 1 : 0);
      if (nd > maxd) continue;
      const int ny = y + dy, nz = z + dz;
      if (ny < 0 || ny >= H || nz < 0) continue;
      const bool rowcross = (dz < 0 && lz == 0) || (dy < 0 && ly == 0) || (dy > 0 && ly == CC_TH - 1);
      const long u = nz * HW + (long)ny * W + x;
      if (CC_RLX_AGENT(&comp[u]) != 0) {
        // left out as in the local kernel; the voxels to the left are joined to these by a run or by the x seam above
        if (rowcross && !(left && CC_RLX_AGENT(&comp[u - 1]) != 0)) cc_union(comp, (int)v, (int)u);
      } else if (nd + 1 <= maxd) {
        if (x > 0 && (rowcross || lane == 0) && CC_RLX_AGENT(&comp[u - 1]) != 0) cc_union(comp, (int)v, (int)u - 1);
        if (x < W - 1 && (rowcross || lane == CC_TW - 1) && CC_RLX_AGENT(&comp[u + 1]) != 0) cc_union(comp, (int)v, (int)u + 1);
      }
    }
  }
}

// ---- flatten: every voxel of the region names its root ---------------------------------------------------------------------------
// In place: a voxel another lane has flattened already names its root, which is an ancestor like any other.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* comp, long n) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int c = CC_RLX_AGENT(&comp[v]);
  if (c == 0 || c == (int)v + 1) return;          // outside the region (0 since the local kernel), or a root: the value stands
  const int root = cc_find(comp, c - 1);
  if (root + 1 != c) __hip_atomic_store(&comp[v], root + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern "C" int bts_components3d(const uint8_t* lab, int* comp, int D, int H, int W, int K, int class_mask, int connectivity,
                                hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || K < 2 || K > CC_MAXK) return BTS_ERR_SHAPE;
  if (class_mask < 0 || class_mask >= (1 << K)) return BTS_ERR_SHAPE;
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) return BTS_ERR_SHAPE;
  const long lim = 0x7fffffffL, dh = (long)D * H;
  if (dh >= lim || dh * W >= lim) return BTS_ERR_SHAPE;                     // index + 1 is an int32
  const long n = dh * W;
  const int ntx = (W + CC_TW - 1) / CC_TW, nty = (H + CC_TH - 1) / CC_TH, ntz = (D + CC_TD - 1) / CC_TD;
  const long tiles = (long)ntx * nty * ntz;                                 // < 2^31: a tile holds a voxel at least
  const int maxd = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
  (void)hipGetLastError();
  hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, lab, comp, D, H, W, ntx, nty, (unsigned)K - 1u,
                     (unsigned)class_mask, maxd);
  BTS_LAUNCH_CHECK();
  if (tiles > 1) {
    hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, comp, D, H, W, ntx, nty, maxd);
    BTS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, comp, n);
    BTS_LAUNCH_CHECK();
  }
  return BTS_OK;
}

// ---- sizes ---------------------------------------------------------------------------------------------------------------------------
// A lane owns CC_CHUNK consecutive elements and merges runs of equal comp before it issues an atomic.  A run of the workgroup's key
// component (the largest comp value among the lanes' first elements: inside a large component, that component) is added in LDS and
// reaches size[] as one atomic per workgroup; every other run is one global integer atomic.  Integer sums commute: exact in every run.
__global__ __launch_bounds__(256) void cc_sizes_kernel(const int* __restrict__ comp, long n, int vec, int* size,
                                                       unsigned long long* ncomp) {
  __shared__ int wg_key;
  __shared__ unsigned wg_cnt, wg_roots;
  if (threadIdx.x == 0) { wg_key = 0; wg_cnt = 0u; wg_roots = 0u; }
  __syncthreads();
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * CC_CHUNK;
  const int m = n - e0 < CC_CHUNK ? (n - e0 < 0 ? 0 : (int)(n - e0)) : CC_CHUNK;
  int c[CC_CHUNK];
  if (vec && m == CC_CHUNK) {
#pragma unroll
    for (int j = 0; j < CC_CHUNK / 4; ++j) {
      const int4 t = *reinterpret_cast<const int4*>(comp + e0 + 4 * j);
      c[4 * j] = t.x; c[4 * j + 1] = t.y; c[4 * j + 2] = t.z; c[4 * j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < CC_CHUNK; ++j) c[j] = j < m ? comp[e0 + j] : 0;
  }
  if (c[0]) atomicMax(&wg_key, c[0]);
  __syncthreads();
  const int key = wg_key;
  int cur = 0, run = 0;
  unsigned roots = 0u;
#pragma unroll
  for (int j = 0; j <= CC_CHUNK; ++j) {
    const int cj = j < CC_CHUNK ? c[j] : 0;
    if (j < CC_CHUNK && cj != 0 && cj == (int)(e0 + j) + 1) ++roots;
    if (cj == cur && j < CC_CHUNK) { ++run; continue; }
    if (cur != 0) {
      if (cur == key) atomicAdd(&wg_cnt, (unsigned)run);
      else atomicAdd(&size[cur - 1], run);
    }
    cur = cj;
    run = 1;
  }
  if (roots) atomicAdd(&wg_roots, roots);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (wg_cnt) atomicAdd(&size[key - 1], (int)wg_cnt);
    if (wg_roots) atomicAdd(ncomp, (unsigned long long)wg_roots);
  }
}

extern "C" int bts_component_sizes(const int* comp, long n, int* size, long* ncomp, hipStream_t stream) {
  if (n < 0 || n >= 0x7fffffffL) return BTS_ERR_SHAPE;
  if (n == 0) return BTS_OK;
  hipError_t e = hipMemsetAsync(size, 0, (size_t)n * sizeof(int), stream);
  if (e != hipSuccess) return (int)e;
  const long per = 256L * CC_CHUNK;
  const int vec = (reinterpret_cast<uintptr_t>(comp) & 15) == 0;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cc_sizes_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(256), 0, stream, comp, n, vec, size,
                     reinterpret_cast<unsigned long long*>(ncomp));
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- largest -------------------------------------------------------------------------------------------------------------------------
// key = (size << 32) | (0xFFFFFFFF - root) orders by size, then by SMALLER root; 0 = no component.  A maximum does not depend on the
// order it is taken in: per lane in a register, per workgroup in LDS, one 64-bit atomicMax per workgroup.
__global__ __launch_bounds__(256) void cc_largest_kernel(const int* __restrict__ size, long n, unsigned long long* key) {
  __shared__ unsigned long long wg_best;
  if (threadIdx.x == 0) wg_best = 0ull;
  __syncthreads();
  unsigned long long best = 0ull;
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (e0 + j < n) {
      const int s = size[e0 + j];
      if (s > 0) {
        const unsigned long long k = ((unsigned long long)(unsigned)s << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(e0 + j));
        best = k > best ? k : best;
      }
    }
  }
  if (best) atomicMax(&wg_best, best);
  __syncthreads();
  if (threadIdx.x == 0 && wg_best) atomicMax(key, wg_best);
}

extern "C" int bts_component_largest(const int* size, long n, uint64_t* key, hipStream_t stream) {
  if (n < 0 || n >= 0x7fffffffL) return BTS_ERR_SHAPE;
  if (n == 0) return BTS_OK;
  hipError_t e = hipMemsetAsync(key, 0, sizeof(uint64_t), stream);
  if (e != hipSuccess) return (int)e;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cc_largest_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, stream, size, n,
                     reinterpret_cast<unsigned long long*>(key));
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------------
// Only voxels of components that fail the predicate are stored to; everything else is left as it is.
__global__ __launch_bounds__(256) void cc_apply_kernel(uint8_t* lab, const int* __restrict__ comp, const int* __restrict__ size,
                                                       const unsigned long long* __restrict__ key, long n, int min_voxels,
                                                       int largest_only, uint8_t fill, unsigned long long* removed_voxels,
                                                       unsigned long long* removed_components) {
  __shared__ unsigned wg_vox, wg_comp;
  if (threadIdx.x == 0) { wg_vox = 0u; wg_comp = 0u; }
  __syncthreads();
  const unsigned keep_root = largest_only ? 0xFFFFFFFFu - (unsigned)(*key & 0xFFFFFFFFull) : 0u;
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  unsigned nv = 0u, nc = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long v = e0 + j;
    if (v < n) {
      const int c = comp[v];
      if (c != 0) {
        const bool keep = size[c - 1] >= min_voxels && (!largest_only || (unsigned)(c - 1) == keep_root);
        if (!keep) {
          lab[v] = fill;
          ++nv;
          if (c == (int)v + 1) ++nc;
        }
      }
    }
  }
  if (nv) atomicAdd(&wg_vox, nv);
  if (nc) atomicAdd(&wg_comp, nc);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (wg_vox) atomicAdd(removed_voxels, (unsigned long long)wg_vox);
    if (wg_comp && removed_components) atomicAdd(removed_components, (unsigned long long)wg_comp);
  }
}

extern "C" int bts_components_apply(uint8_t* lab, const int* comp, const int* size, const uint64_t* key, long n, int min_voxels,
                                    int largest_only, int fill, long* removed_voxels, long* removed_components, hipStream_t stream) {
  if (n < 0 || n >= 0x7fffffffL || min_voxels < 0 || fill < 0 || fill > 255) return BTS_ERR_SHAPE;
  if (largest_only && key == nullptr) return BTS_ERR_SHAPE;
  if (n == 0) return BTS_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cc_apply_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, stream, lab, comp, size,
                     reinterpret_cast<const unsigned long long*>(key), n, min_voxels, largest_only ? 1 : 0, (uint8_t)fill,
                     reinterpret_cast<unsigned long long*>(removed_voxels), reinterpret_cast<unsigned long long*>(removed_components));
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- relabel a small region -----------------------------------------------------------------------------------------------------------
// confusion: the K x K counts bts_label_confusion(lab, lab) gave, on the device: the region's voxel count is the sum of its classes'
// diagonal entries, read by every lane (a broadcast), so the decision needs no host round trip.
__global__ __launch_bounds__(256) void cc_relabel_kernel(uint8_t* lab, long n, int K, unsigned class_mask, uint8_t fill,
                                                         const long* __restrict__ confusion, long limit,
                                                         unsigned long long* changed) {
  long count = 0;
  for (int c = 0; c < K; ++c)
    if ((class_mask >> c) & 1u) count += confusion[c * K + c];
  if (count <= 0 || count >= limit) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(changed, (unsigned long long)count);
  const unsigned top = (unsigned)K - 1u;
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e0 + j < n && cc_in_region(lab[e0 + j], top, class_mask)) lab[e0 + j] = fill;
}

extern "C" int bts_region_relabel(uint8_t* lab, long n, int K, int class_mask, int fill, const long* confusion, long limit,
                                  long* changed, hipStream_t stream) {
  if (n < 0 || n > (1L << 40) || K < 2 || K > CC_MAXK || class_mask < 0 || class_mask >= (1 << K) || fill < 0 || fill > 255 || limit < 0)
    return BTS_ERR_SHAPE;
  if (n == 0 || limit == 0) return BTS_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cc_relabel_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, stream, lab, n, K, (unsigned)class_mask,
                     (uint8_t)fill, confusion, limit, reinterpret_cast<unsigned long long*>(changed));
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
