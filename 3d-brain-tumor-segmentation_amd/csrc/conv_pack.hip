// Weight packing for the fp32 conv engine (role = forward or data-gradient), and the registry of which parts of a K3S1 image are read.
// Source layouts are the reference's Keras layouts:
// Conv3D (kd,kh,kw,Cin,Cout) -- resnet.py:30-37,80-87; Conv3DTranspose (kd,kh,kw,Cout,Cin) -- upsample.py:28-33.
// The encoder's dense connections feed block j the list [o_{j-1}, o_0..o_{j-1}] (encoder.py:83-87): the
// duplicated slice is folded here (Wp = W[first copy] + W[second copy]) so the kernel reads the level slab
// [o_0..o_{j-1}] once.  The implicit-GEMM layout Wp[tap][kgroup(8 ch)][half][Npad][4] is described in conv_igemm.hip; a K3S1 image
// carries two Winograd-domain parts behind it (conv_wino.hip, conv_wino3.hip).
#include <stdlib.h>
#include <mutex>
#include <unordered_map>
#include "common.h"
#include "conv_plan.h"

struct PackParams {
  const float* w;
  float* wp;
  int ntaps, K, N, KG, Npad;
  long sT, sK, sN;  // source strides for (tap, k, n)
  int flip;         // tap t reads source tap ntaps-1-t
  int cin_is_k;     // 1: the (possibly folded) input-channel axis is k, 0: it is n, -1: no fold
  int shift, dup_start;
  long wino_off;    // K3S1 images: element index where the Winograd part starts; otherwise beyond the image
  long w3_item0;    // K3S1 images: first work item of the 3-D Winograd part (conv_wino3.hip); its floats start at w3_off
  long w3_off;
  long total;       // floats of the whole image
  long items;       // work items (pack_item): implicit-GEMM floats + Winograd positions (16 floats each), of the parts in `parts` only
  unsigned parts;   // K3S1 images: which of the three parts this pack writes (IMG_IGEMM | IMG_WINO | IMG_W3); IMG_ALL otherwise
};
// index into the items of the enabled parts -> work item of the whole image
__device__ __forceinline__ long pack_map(const PackParams& q, long j) {
  if (q.parts == IMG_ALL) return j;
  const long n0 = (q.parts & IMG_IGEMM) ? q.wino_off : 0;
  if (j < n0) return j;
  j -= n0;
  const long n1 = (q.parts & IMG_WINO) ? (q.w3_item0 - q.wino_off) : 0;
  if (j < n1) return q.wino_off + j;
  return q.w3_item0 + (j - n1);
}

// source value of packed position (tap t, contraction index k, column n), with the tap flip of the data-gradient role and
// the encoder's duplicated input slice folded in
__device__ __forceinline__ float pack_src(const PackParams& q, int t, int k, int n) {
  if (k >= q.K || n >= q.N) return 0.f;
  const int ts = q.flip ? (q.ntaps - 1 - t) : t;
  int kk = k, nn = n, k2 = -1, n2 = -1;
  if (q.cin_is_k == 1) {
    if (k >= q.dup_start) k2 = k - q.dup_start;
    kk = k + q.shift;
    n2 = n;
  } else if (q.cin_is_k == 0) {
    if (n >= q.dup_start) n2 = n - q.dup_start;
    nn = n + q.shift;
    k2 = k;
  }
  float v = q.w[ts * q.sT + kk * q.sK + nn * q.sN];
  if (q.shift > 0 && k2 >= 0 && n2 >= 0) v += q.w[ts * q.sT + k2 * q.sK + n2 * q.sN];
  return v;
}

// One work item of an image: index i < wino_off writes one float of the implicit-GEMM part; an index above it writes the
// 16 transform points of one (cout block, k-group, x tap, half, cout, cin) position of the Winograd part (conv_wino.hip):
// U = G g G^T over the (z, y) taps, layout [cout block of 32][k-group][x tap][xi_z*4 + xi_y][half][32][4]; the 9 source
// taps are read once.  rows of G: (1 0 0) (.5 .5 .5) (.5 -.5 .5) (0 0 1)
__device__ __forceinline__ float pack_g_(int r, float g0, float g1, float g2) {   // row r of G applied to three taps
  return r == 0 ? g0 : r == 1 ? fmaf(0.5f, g2, fmaf(0.5f, g1, 0.5f * g0)) : r == 2 ? fmaf(0.5f, g2, fmaf(-0.5f, g1, 0.5f * g0)) : g2;
}
__device__ __forceinline__ void pack_item(const PackParams& q, long i) {
  if (i >= q.w3_item0) {
    // third part: U = (G x G x G) g over all 27 taps, 64 transform points xi = (xi_z*4 + xi_y)*4 + xi_x per (cin, cout) pair,
    // layout [cout block of 32][k-group of 8 cin][xi][half][32 couts][4 cin] (conv_wino3.hip)
    long r = i - q.w3_item0;
    const int j = (int)(r & 3);
    const int n32 = (int)((r >> 2) & 31);
    const int hh = (int)((r >> 7) & 1);
    r >>= 8;
    const int kg = (int)(r % q.KG);
    const int cb = (int)(r / q.KG);
    const int k = kg * 8 + hh * 4 + j, n = cb * 32 + n32;
    float t[4][3][3], u[4][4][3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float g0 = pack_src(q, (0 * 3 + ky) * 3 + kx, k, n), g1 = pack_src(q, (1 * 3 + ky) * 3 + kx, k, n),
                    g2 = pack_src(q, (2 * 3 + ky) * 3 + kx, k, n);
#pragma unroll
        for (int a = 0; a < 4; ++a) t[a][ky][kx] = pack_g_(a, g0, g1, g2);
      }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int b = 0; b < 4; ++b) u[a][b][kx] = pack_g_(b, t[a][0][kx], t[a][1][kx], t[a][2][kx]);
    float* o = q.wp + q.w3_off + (((long)cb * q.KG + kg) * 64) * 256 + hh * 128 + n32 * 4 + j;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) o[((a * 4 + b) * 4 + c) * 256] = pack_g_(c, u[a][b][0], u[a][b][1], u[a][b][2]);
    return;
  }
  if (i >= q.wino_off) {
    long r = i - q.wino_off;
    const int j = (int)(r & 3);
    const int n32 = (int)((r >> 2) & 31);
    const int hh = (int)((r >> 7) & 1);
    r >>= 8;
    const int dx = (int)(r % 3); r /= 3;
    const int kg = (int)(r % q.KG);
    const int cb = (int)(r / q.KG);
    const int k = kg * 8 + hh * 4 + j, n = cb * 32 + n32;
    float g[3][3], t[4][3];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) g[kz][ky] = pack_src(q, (kz * 3 + ky) * 3 + dx, k, n);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {  // G along z
      t[0][ky] = g[0][ky];
      t[1][ky] = fmaf(0.5f, g[2][ky], fmaf(0.5f, g[1][ky], 0.5f * g[0][ky]));
      t[2][ky] = fmaf(0.5f, g[2][ky], fmaf(-0.5f, g[1][ky], 0.5f * g[0][ky]));
      t[3][ky] = g[2][ky];
    }
    float* o = q.wp + q.wino_off + ((((long)cb * q.KG + kg) * 3 + dx) * 16) * 256 + hh * 128 + n32 * 4 + j;
#pragma unroll
    for (int xz = 0; xz < 4; ++xz) {  // G along y
      o[(xz * 4 + 0) * 256] = t[xz][0];
      o[(xz * 4 + 1) * 256] = fmaf(0.5f, t[xz][2], fmaf(0.5f, t[xz][1], 0.5f * t[xz][0]));
      o[(xz * 4 + 2) * 256] = fmaf(0.5f, t[xz][2], fmaf(-0.5f, t[xz][1], 0.5f * t[xz][0]));
      o[(xz * 4 + 3) * 256] = t[xz][2];
    }
    return;
  }
  const int j = (int)(i & 3);
  long r = i >> 2;
  const int n = (int)(r % q.Npad); r /= q.Npad;
  const int hh = (int)(r & 1); r >>= 1;
  const int kg = (int)(r % q.KG);
  const int t = (int)(r / q.KG);
  q.wp[i] = pack_src(q, t, kg * 8 + hh * 4 + j, n);
}

__global__ void pack_kernel(const PackParams q) {
  const long total = q.items;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    pack_item(q, pack_map(q, i));
}

// All layers' weight images in one launch (the optimiser step invalidates every image at once; 120 separate 5 us
// launches per training step otherwise).  Descriptor table in device memory, block -> entry by binary search.
#define PACK_BLOCK_ELEMS 2048
struct PackDesc {
  PackParams q;
  long first_block, total;
};
__global__ __launch_bounds__(256) void pack_batch_kernel(const PackDesc* __restrict__ descs, int n) {
  int lo = 0, hi = n - 1;
  const long b = blockIdx.x;
  while (lo < hi) {  // last entry with first_block <= b
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  const PackDesc d = descs[lo];
  const long i0 = (b - d.first_block) * PACK_BLOCK_ELEMS;
#pragma unroll
  for (int u = 0; u < PACK_BLOCK_ELEMS / 256; ++u) {
    const long i = i0 + threadIdx.x + u * 256;
    if (i < d.total) pack_item(d.q, pack_map(d.q, i));
  }
}

extern "C" long bts_conv_packed_floats(int kind, int role, int Cin, int Cout) {
  const int ntaps = (kind == BTS_CONV_K1) ? 1 : 27;
  const int K = (role == BTS_ROLE_FWD) ? Cin : Cout;
  const int N = (role == BTS_ROLE_FWD) ? Cout : Cin;
  // K3S1 images carry two Winograd-domain copies: 16 transform points x 3 x taps (conv_wino.hip), 64 points (conv_wino3.hip)
  return (long)(ntaps + (kind == BTS_CONV_K3S1 ? 48 + 64 : 0)) * ((K + 7) / 8) * 2 * conv_npad32(N) * 4;
}

static int pack_params(PackParams& q, int kind, int role, const float* w, float* wp, int Cin_ref, int Cout, int Cin_slab,
                       int dup_start, int dup_shift, unsigned parts = IMG_ALL) {
  if (kind < 0 || kind > 3 || role < 0 || role > 1) return BTS_ERR_UNSUPPORTED;
  if (dup_shift > 0 && (kind == BTS_CONV_K3S2 || kind == BTS_CONV_K3S2T)) return BTS_ERR_UNSUPPORTED;
  if (Cin_slab + dup_shift != Cin_ref) return BTS_ERR_SHAPE;
  q.w = w;
  q.wp = wp;
  q.ntaps = (kind == BTS_CONV_K1) ? 1 : 27;
  q.shift = dup_shift;
  q.dup_start = dup_shift > 0 ? dup_start : (1 << 30);
  long sCin, sCout;
  if (kind == BTS_CONV_K3S2T) { sCout = Cin_ref; sCin = 1; }  // (t, Cout, Cin)
  else { sCin = Cout; sCout = 1; }                            // (t, Cin, Cout)
  q.sT = (long)Cin_ref * Cout;
  if (role == BTS_ROLE_FWD) {
    q.K = Cin_slab; q.N = Cout; q.sK = sCin; q.sN = sCout; q.flip = 0; q.cin_is_k = 1;
  } else {
    q.K = Cout; q.N = Cin_slab; q.sK = sCout; q.sN = sCin; q.cin_is_k = 0;
    q.flip = (kind == BTS_CONV_K3S1) ? 1 : 0;
  }
  q.KG = (q.K + 7) / 8;
  q.Npad = conv_npad32(q.N);
  const long ig = (long)q.ntaps * q.KG * 2 * q.Npad * 4;
  q.wino_off = (kind == BTS_CONV_K3S1) ? ig : (1L << 62);
  const long pairs = (long)q.KG * 2 * q.Npad * 4;   // (contraction index, column) pairs of the padded image
  q.total = ig + ((kind == BTS_CONV_K3S1) ? (48L + 64L) * pairs : 0L);
  q.w3_item0 = (kind == BTS_CONV_K3S1) ? ig + 3L * pairs : (1L << 62);
  q.w3_off = ig + 48L * pairs;
  q.parts = IMG_ALL;
  q.items = ig + ((kind == BTS_CONV_K3S1) ? (3L + 1L) * pairs : 0L);
  if (kind == BTS_CONV_K3S1 && (parts & IMG_ALL) != IMG_ALL && (parts & IMG_ALL) != 0u) {
    q.parts = parts & IMG_ALL;
    q.items = ((q.parts & IMG_IGEMM) ? ig : 0L) + ((q.parts & IMG_WINO) ? 3L * pairs : 0L) + ((q.parts & IMG_W3) ? pairs : 0L);
  }
  return BTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Which parts of a K3S1 image are READ.  An image carries three forms of the same weights (139 floats per (cin, cout) pair: 27 + 48 +
// 64) and a layer uses ONE of them at a given geometry -- re-packing all three after every optimiser step wrote ~1.6 GB per fp32
// training step (pack_batch_kernel 0.67-0.77 ms, round-4 review).  The library therefore keeps, per image (keyed by its base address),
// the parts the dispatcher has picked so far (`used`, recorded right before each launch), and descriptor tables are built for those
// parts only (`table_mask`).  A launch that picks a part no table covers packs it on the spot, on its own stream, from the recorded
// source (`fresh_extra` remembers that until the next batch pack, i.e. the next weight change), and bumps the generation counter so that
// the host rebuilds its table (ops.PackTable) at the next re-pack.  bts_conv_pack (single image, all parts) is how images are born.
// ---------------------------------------------------------------------------------------------
struct ImgState {
  int kind, role, Cin_ref, Cout, Cin_slab, dup_start, dup_shift;
  const float* w;
  unsigned used, table_mask, fresh_extra;
};
static std::mutex g_img_mu;
static std::unordered_map<const void*, ImgState> g_img;
static long g_img_gen = 0;
static bool img_masks_enabled() {   // BTS_PACK_USED=0: every pack writes all three parts (A/B; read per call)
  const char* e = getenv("BTS_PACK_USED");
  return !(e && atoi(e) == 0);
}
// (re)register an image; returns the parts a table built now should describe.  table_mask is what the table LAST RUN on the image
// wrote (set by bts_conv_pack_batch from the host copy of that table), never what some table merely describes: with two tables for one
// image, or a cached narrow table behind a bts_conv_pack of the whole image, the parts a batch did NOT write must go stale (round-5
// advisor finding: a re-registration through bts_conv_pack used to mark all three parts as table-covered).
static unsigned img_register(const float* wp, int kind, int role, const float* w, int Cin_ref, int Cout, int Cin_slab, int dup_start,
                             int dup_shift, bool all_parts) {
  std::lock_guard<std::mutex> lk(g_img_mu);
  ImgState& e = g_img[wp];
  const bool same = e.w == w && e.kind == kind && e.role == role && e.Cin_ref == Cin_ref && e.Cout == Cout && e.Cin_slab == Cin_slab &&
                    e.dup_start == dup_start && e.dup_shift == dup_shift;
  if (!same) { e = ImgState{kind, role, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, w, 0u, 0u, 0u}; }      // (another image at this address: nothing is known)
  if (all_parts) {      // bts_conv_pack writes every part: all fresh until the next batch re-pack over this image
    e.fresh_extra = IMG_ALL;
    return IMG_ALL;
  }
  unsigned m = IMG_ALL;
  if (kind == BTS_CONV_K3S1 && e.used != 0u && img_masks_enabled()) m = e.used;
  return m;
}
extern "C" long bts_conv_pack_generation(void) {
  std::lock_guard<std::mutex> lk(g_img_mu);
  return g_img_gen;
}
extern "C" int bts_conv_pack_forget(const float* wp) {      // the image's memory is being released: drop its registry entry
  std::lock_guard<std::mutex> lk(g_img_mu);
  return g_img.erase(wp) ? 1 : 0;
}
// Called right before a kernel reads part `bit` of the K3S1 image at `base`: packs the part on `stream` from the recorded source when the
// last re-pack left it out.  The part counts as fresh only after the pack launch was accepted; an error is the caller's to return.
int bts_img_ensure_(const float* base, unsigned bit, hipStream_t stream) {
  PackParams q;
  {
    std::lock_guard<std::mutex> lk(g_img_mu);
    auto it = g_img.find(base);
    if (it == g_img.end() || it->second.kind != BTS_CONV_K3S1) return BTS_OK;      // (an image this registry never saw: packed whole by its owner)
    const ImgState& e = it->second;
    if ((e.table_mask | e.fresh_extra) & bit) return BTS_OK;
    const int r = pack_params(q, e.kind, e.role, e.w, const_cast<float*>(base), e.Cin_ref, e.Cout, e.Cin_slab, e.dup_start, e.dup_shift, bit);
    if (r != BTS_OK) return r;
  }
  long blocks = (q.items + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  (void)hipGetLastError();
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, q);
  BTS_LAUNCH_CHECK();
  std::lock_guard<std::mutex> lk(g_img_mu);
  auto it = g_img.find(base);
  if (it != g_img.end()) it->second.fresh_extra |= bit;
  return BTS_OK;
}
// a launcher has ACCEPTED a launch that reads part `bit`: descriptor tables built from now on describe it (generation moves once per new form)
void bts_img_mark_used_(const float* base, unsigned bit) {
  std::lock_guard<std::mutex> lk(g_img_mu);
  auto it = g_img.find(base);
  if (it == g_img.end() || it->second.kind != BTS_CONV_K3S1) return;
  if (!(it->second.used & bit)) { it->second.used |= bit; ++g_img_gen; }
}

extern "C" int bts_conv_pack(int kind, int role, const float* w, float* wp, int Cin_ref, int Cout, int Cin_slab,
                             int dup_start, int dup_shift, hipStream_t stream) {
  PackParams q;
  const int r = pack_params(q, kind, role, w, wp, Cin_ref, Cout, Cin_slab, dup_start, dup_shift);
  if (r != BTS_OK) return r;
  if (w != nullptr && wp != nullptr) img_register(wp, kind, role, w, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, true);
  const long total = q.items;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  (void)hipGetLastError(); hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(256), 0, stream, q);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

extern "C" long bts_conv_pack_desc_bytes(void) { return (long)sizeof(PackDesc); }

// Fill descriptor #index of a HOST table (bts_conv_pack_desc_bytes() bytes per entry); first_block = sum of the block
// counts returned for the entries before it.  Returns this entry's block count (> 0) or a negative engine code.
extern "C" long bts_conv_pack_desc(void* host_table, int index, long first_block, int kind, int role, const float* w, float* wp,
                                   int Cin_ref, int Cout, int Cin_slab, int dup_start, int dup_shift) {
  PackDesc d;
  int r = pack_params(d.q, kind, role, w, wp, Cin_ref, Cout, Cin_slab, dup_start, dup_shift);
  if (r != BTS_OK) return r;
  const unsigned parts = img_register(wp, kind, role, w, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, false);   // (the parts read so far; all when none yet)
  if (parts != IMG_ALL) r = pack_params(d.q, kind, role, w, wp, Cin_ref, Cout, Cin_slab, dup_start, dup_shift, parts);
  if (r != BTS_OK) return r;
  d.total = d.q.items;
  d.first_block = first_block;
  reinterpret_cast<PackDesc*>(host_table)[index] = d;
  return (d.total + PACK_BLOCK_ELEMS - 1) / PACK_BLOCK_ELEMS;
}

// table_dev: the host table copied to device memory by the caller; table_host: that host table (still readable; may be NULL);
// total_blocks = sum of all block counts.  A batch pack follows a weight change: for every image IN THE TABLE the parts this table
// writes are fresh afterwards and every other part is stale (packed on demand at its next use).  Without the host copy the library cannot
// know which images / parts the table covers: every registered image then counts as stale in every part (correct, but each K3S1 launch
// re-packs its part once per weight change).
extern "C" int bts_conv_pack_batch(const void* table_dev, const void* table_host, int n, long total_blocks, hipStream_t stream) {
  if (n <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffL) return BTS_ERR_SHAPE;
  {
    std::lock_guard<std::mutex> lk(g_img_mu);
    if (table_host != nullptr) {
      const PackDesc* t = reinterpret_cast<const PackDesc*>(table_host);
      for (int i = 0; i < n; ++i) {
        auto it = g_img.find(t[i].q.wp);
        if (it == g_img.end()) continue;
        it->second.table_mask = (it->second.kind == BTS_CONV_K3S1) ? (t[i].q.parts & IMG_ALL) : IMG_ALL;
        it->second.fresh_extra = 0u;
      }
    } else {
      for (auto& kv : g_img) { kv.second.table_mask = 0u; kv.second.fresh_extra = 0u; }
    }
  }
  (void)hipGetLastError(); hipLaunchKernelGGL(pack_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, stream,
                     reinterpret_cast<const PackDesc*>(table_dev), n);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
