// Weight gradient of the 1x1x1 convs (the ResNet blocks' shortcut convs, resnet.py:96-103, and the decoder / VAE projections):
// dW[c][k] = sum_v P[v][c] * Q[v][k] -- a 32x32 tile per (P, Q) channel-group pair with K = all voxels: 2 FLOP per loaded
// byte, HBM-bound.  The staged kernel (LDS DMA, a barrier per 256-voxel sub-tile, 8 matrix instructions between barriers) ran
// these at ~2 TB/s.  Here nothing is staged: the MFMA operand layout (lane = channel, register = voxel of the K pair) is
// exactly a coalesced 128-byte row read, so each lane streams its channel of consecutive voxels with 16 independent 4-byte
// loads in flight and feeds them to the matrix pipe directly; 8 waves per workgroup split the workgroup's voxel range and
// are summed in LDS in fixed order.  Bias partials (column sums of Q) fall out of the B operands.
#include "wgrad_plan.h"

#define K1W_THREADS WG_THREADS
#define K1W_U 8
__global__ __launch_bounds__(K1W_THREADS, 2) void k1w_kernel(const WgradParams p, long NV, long chunk) {
  __shared__ float lds[WG_WAVES * 1024];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch = lane & 31, hh = lane >> 5;
  const int pct = blockIdx.y, qct = blockIdx.z;
  const int pc = pct * 32 + ch, qc = qct * 32 + ch;
  const bool pok = pc < p.Cp, qok = qc < p.Cq;
  const long w0 = (long)blockIdx.x * chunk;
  long w1 = w0 + chunk;
  if (w1 > NV) w1 = NV;
  // this wave's part of the workgroup range, whole K pairs
  long per = ((w1 - w0 + 7) / 8 + 1) & ~1L;
  long v = w0 + wave * per;
  long ve = v + per;
  if (ve > w1) ve = w1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  double bsum = 0.0;
  const bool bias = p.want_bias && pct == 0;
  const float* pp = p.p + pc;
  const float* qq = p.q + qc;
  for (; v < ve; v += 2 * K1W_U) {
    float a[K1W_U], b[K1W_U];
#pragma unroll
    for (int u = 0; u < K1W_U; ++u) {
      const long vv = v + 2 * u + hh;
      const bool in = vv < ve;
      a[u] = (in && pok) ? pp[vv * p.ldp] : 0.f;
      b[u] = (in && qok) ? qq[vv * p.ldq] : 0.f;
    }
    float bs = 0.f;
#pragma unroll
    for (int u = 0; u < K1W_U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
      bs += b[u];
    }
    if (bias) bsum += (double)bs;
  }
  // fixed-order sum of the 8 waves' tiles
#pragma unroll
  for (int r = 0; r < 16; ++r) lds[wave * 1024 + wg_acc_row(r, hh) * 32 + ch] = acc[r];
  __syncthreads();
  // (= wg_partial_base(pct, qct, p.ntiles), which compiles to another instruction order here)
  float* dst = p.partial + ((((long)blockIdx.x * gridDim.y + pct) * gridDim.z + qct) * p.ntiles) * 1024;
  for (int e = tid; e < 1024; e += K1W_THREADS) {
    float sacc = lds[e];
#pragma unroll
    for (int w = 1; w < 8; ++w) sacc += lds[w * 1024 + e];
    dst[e] = sacc;
  }
  if (bias) wg_bias_partial(lds, bsum, p, qct, tid);   // bsum of thread [wave][hh][ch]
}

// chunk: the voxels of one workgroup, whole 16s
int bts_k1w_launch_(const WgChoice& ch, const WgradParams& p, hipStream_t stream) {
  const long chunk = (((ch.NV + ch.nsp - 1) / ch.nsp) + 15) & ~15L;
  const bool prof = bts_prof_on();
  if (prof) bts_prof_begin(ch.sym, ch.flops, stream);
  (void)hipGetLastError();
  hipLaunchKernelGGL(k1w_kernel, dim3(ch.nsp, ch.npct, ch.nqct), dim3(K1W_THREADS), 0, stream, p, ch.NV, chunk);
  if (prof) bts_prof_end(stream);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
