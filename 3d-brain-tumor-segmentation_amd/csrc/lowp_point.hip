// Element-wise and per-voxel passes of the 16-bit engine: casts between fp32 and the storage type (dropout + cast included), the
// non-default samplers (max-pool, nearest up-sample) with their gradients, the output head and its backward, and the fixed-order row
// adder lp_dbias_finalize_kernel behind every bias gradient that leaves a backward pass as per-block partial rows.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.h"
#include "bts_internal.h"
#include "lowp_common.h"
#include "finalize_parts.h"

// =====================================================================================================================
// element-wise passes of the forward (16-bit in / out, fp32 arithmetic)
// =====================================================================================================================
// fp32 -> storage type, rows of C elements with row strides (elements)
template <typename T>
__global__ __launch_bounds__(256) void lp_cast_kernel(const float* src, long lds_, unsigned short* dst, long ldd, long rows, int C) {
  const long total = rows * C;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    dst[r * ldd + c] = T::st(src[r * lds_ + c]);
  }
}
// rows of a few channels (the 2-channel volume into its 16-channel matrix step, the 1- and 2-channel VAE tensors): a thread per row --
// the element form spends a 64-bit division per 2 bytes
template <typename T, int C>
__global__ __launch_bounds__(256) void lp_cast_rows_kernel(const float* __restrict__ src, long lds_, unsigned short* __restrict__ dst, long ldd, long rows) {
  for (long r = blockIdx.x * 256L + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = src[r * lds_ + c];
    if constexpr (C % 2 == 0) {
#pragma unroll
      for (int c = 0; c < C; c += 2) *reinterpret_cast<unsigned*>(dst + r * ldd + c) = pack2<T>(v[c], v[c + 1]);      // (ldd and the view's first channel even)
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) dst[r * ldd + c] = T::st(v[c]);
    }
  }
}
extern "C" int bts_lp_cast(int dtype, const float* src, long ld_src, void* dst, long ld_dst, long rows, int C, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (rows <= 0 || C <= 0) return BTS_ERR_SHAPE;
  (void)hipGetLastError();
  if (C <= 4 && (C % 2 != 0 || (ld_dst % 2 == 0 && (((uintptr_t)dst) & 3) == 0))) {
    long rb = (rows + 255) / 256;
    if (rb > 65536) rb = 65536;
#define LP_CR(T_, C_) hipLaunchKernelGGL((lp_cast_rows_kernel<T_, C_>), dim3((unsigned)rb), dim3(256), 0, stream, src, ld_src, (unsigned short*)dst, ld_dst, rows)
    lp_typed(dtype, [&](auto t) {
      using T = decltype(t);
      if (C == 1) LP_CR(T, 1); else if (C == 2) LP_CR(T, 2); else if (C == 3) LP_CR(T, 3); else LP_CR(T, 4);
    });
#undef LP_CR
    BTS_LAUNCH_CHECK();
    return BTS_OK;
  }
  long blocks = (rows * C + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_cast_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, stream, src, ld_src, (unsigned short*)dst, ld_dst, rows, C);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
template <typename T>
__global__ __launch_bounds__(256) void lp_uncast_kernel(const unsigned short* src, long lds_, float* dst, long ldd, long rows, int C) {
  const long total = rows * C;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    dst[r * ldd + c] = T::ld(src[r * lds_ + c]);
  }
}
// fp32 rows of C (<= 4) channels -> storage-type rows of 16 channels, the tail zero: the 2-channel volume / VAE-output gradient and
// the 1-channel VAE tensor as whole matrix steps in ONE pass (a zero fill of the 16-channel tensor + bts_lp_cast into its first
// channels wrote every row twice: 0.28 ms per 8 x 128^3 tensor)
template <typename T, int C>
__global__ __launch_bounds__(256) void lp_cast_pad16_kernel(const float* __restrict__ src, long lds_, unsigned short* __restrict__ dst, long rows) {
  for (long r = blockIdx.x * 256L + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = src[r * lds_ + c];
    u32x4* o = reinterpret_cast<u32x4*>(dst + r * 16);
    o[0] = u32x4{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), 0u, 0u};
    o[1] = u32x4{0u, 0u, 0u, 0u};
  }
}
extern "C" int bts_lp_cast_pad16(int dtype, const float* src, long ld_src, void* dst, long rows, int C, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (rows <= 0 || C <= 0 || C > 4 || ld_src < C) return BTS_ERR_SHAPE;
  if (((uintptr_t)dst) & 15) return BTS_ERR_ALIGN;
  long blocks = (rows + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  (void)hipGetLastError();
#define LP_CP(TT, C_) hipLaunchKernelGGL((lp_cast_pad16_kernel<TT, C_>), dim3((unsigned)blocks), dim3(256), 0, stream, src, ld_src, (unsigned short*)dst, rows)
  lp_typed(dtype, [&](auto t) {
    using T = decltype(t);
    if (C == 1) LP_CP(T, 1); else if (C == 2) LP_CP(T, 2); else if (C == 3) LP_CP(T, 3); else LP_CP(T, 4);
  });
#undef LP_CP
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
// The input dropout of the encoder (encoder.py:39,71: Dropout(0.2) on the 2-channel volume) AND the cast into the zero-padded 16-channel
// matrix step in ONE pass: element i of the dense (rows, C) fp32 volume is kept (and scaled by 1 / (1 - rate)) where the counter-based
// generator of bts_dropout_mask says so -- the SAME draw, element for element (u01(seed, i) >= rate) -- so the result equals
// bts_dropout_mask + bts_dropout_apply + bts_lp_cast_pad16 bit for bit, without the mask and the dropped fp32 volume ever being written
// (three launches, 0.30 ms per 8 x 128^3 step -> one).  The first block's input has no gradient: nothing downstream needs the mask.
template <typename T, int C>
__global__ __launch_bounds__(256) void lp_dropout_cast_pad16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long rows, float rate,
                                                                    float scale, uint64_t seed) {
  for (long r = blockIdx.x * 256L + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < C; ++c) {
      // (the product must be rounded to fp32 BEFORE the cast, as the three-pass route stores it: left to the compiler -- __fmul_rn
      // included -- multiply and fp16 conversion become one mixed-precision instruction, rounded once: 1 element in 30,000 differs)
      float pr = src[r * C + c] * scale;
      asm volatile("" : "+v"(pr));
      v[c] = u01(seed, (uint64_t)(r * C + c)) >= rate ? pr : 0.f;
    }
    u32x4* o = reinterpret_cast<u32x4*>(dst + r * 16);
    o[0] = u32x4{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), 0u, 0u};
    o[1] = u32x4{0u, 0u, 0u, 0u};
  }
}
extern "C" int bts_lp_dropout_cast_pad16(int dtype, const float* src, void* dst, long rows, int C, float rate, uint64_t seed, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (rows <= 0 || C <= 0 || C > 4 || rate < 0.f || rate >= 1.f) return BTS_ERR_SHAPE;
  if (((uintptr_t)dst) & 15) return BTS_ERR_ALIGN;
  long blocks = (rows + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const float scale = 1.0f / (1.0f - rate);
  (void)hipGetLastError();
#define LP_DCP(TT, C_) hipLaunchKernelGGL((lp_dropout_cast_pad16_kernel<TT, C_>), dim3((unsigned)blocks), dim3(256), 0, stream, src, (unsigned short*)dst, rows, rate, scale, seed)
  lp_typed(dtype, [&](auto t) {
    using T = decltype(t);
    if (C == 1) LP_DCP(T, 1); else if (C == 2) LP_DCP(T, 2); else if (C == 3) LP_DCP(T, 3); else LP_DCP(T, 4);
  });
#undef LP_DCP
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
extern "C" int bts_lp_uncast(int dtype, const void* src, long ld_src, float* dst, long ld_dst, long rows, int C, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (rows <= 0 || C <= 0) return BTS_ERR_SHAPE;
  long blocks = (rows * C + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_uncast_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, stream, (const unsigned short*)src, ld_src, dst, ld_dst, rows, C);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- the non-default samplers on 16-bit tensors (args.py:136-141): MaxPooling3D(2) (downsample.py:51-70) and
// UpSampling3D(2) = nearest-neighbour repeat (upsample.py:69), with their gradients (train.py:142-151 under TF autodiff).  Eight
// channels (one 16-byte piece) per thread; the pool keeps the window position of the FIRST maximum (scan order dz, dy, dx) like the
// fp32 engine's bts_maxpool2_fwd, so that the gradient routing is the same; sums of the repeat's gradient run in fp32.
template <typename T>
__global__ __launch_bounds__(256) void lp_maxpool2_fwd_kernel(const unsigned short* x, unsigned short* y, unsigned char* idx, long total8, int Do,
                                                              int Ho, int Wo, int C, int ldx, int ldy) {
  const int C8 = C >> 3;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total8; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C8) * 8;
    long v = i / C8;
    const int ox = (int)(v % Wo); v /= Wo;
    const int oy = (int)(v % Ho); v /= Ho;
    const int oz = (int)(v % Do);
    const long n = v / Do;
    float best[8];
    unsigned char bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const long src = (((n * (2 * Do) + 2 * oz + (t >> 2)) * (2 * Ho) + 2 * oy + ((t >> 1) & 1)) * (2L * Wo) + 2 * ox + (t & 1));
      float f[8];
      unpack8<T>(*reinterpret_cast<const u32x4*>(x + src * ldx + c), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) if (f[e] > best[e]) { best[e] = f[e]; bi[e] = (unsigned char)t; }
    }
    const long dst = ((n * Do + oz) * Ho + oy) * (long)Wo + ox;
    *reinterpret_cast<u32x4*>(y + dst * ldy + c) = pack8<T>(best);
    if (idx != nullptr) {
      unsigned lo = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24), hi = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
      *reinterpret_cast<u32x2*>(idx + dst * C + c) = u32x2{lo, hi};
    }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void lp_maxpool2_bwd_kernel(const unsigned short* dy, const unsigned char* idx, unsigned short* dx, long total8,
                                                              int Do, int Ho, int Wo, int C, int lddy, int lddx, int accum) {
  const int C8 = C >> 3;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total8; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C8) * 8;
    long v = i / C8;
    const int ox = (int)(v % Wo); v /= Wo;
    const int oy = (int)(v % Ho); v /= Ho;
    const int oz = (int)(v % Do);
    const long n = v / Do;
    const long src = ((n * Do + oz) * Ho + oy) * (long)Wo + ox;
    float g[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(dy + src * lddy + c), g);
    const u32x2 pk = *reinterpret_cast<const u32x2*>(idx + src * C + c);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const long dst = (((n * (2 * Do) + 2 * oz + (t >> 2)) * (2 * Ho) + 2 * oy + ((t >> 1) & 1)) * (2L * Wo) + 2 * ox + (t & 1));
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (((e < 4 ? pk[0] >> (8 * e) : pk[1] >> (8 * (e - 4))) & 0xffu) == (unsigned)t) ? g[e] : 0.f;
      if (accum) {
        float old[8];
        unpack8<T>(*reinterpret_cast<const u32x4*>(dx + dst * lddx + c), old);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += old[e];
      }
      *reinterpret_cast<u32x4*>(dx + dst * lddx + c) = pack8<T>(o);
    }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void lp_upsample2_fwd_kernel(const unsigned short* x, unsigned short* y, long total8, int D, int H, int W, int C,
                                                               int ldx, int ldy) {
  const int C8 = C >> 3;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total8; i += (long)gridDim.x * 256) {      // over the FINE grid
    const int c = (int)(i % C8) * 8;
    long v = i / C8;
    const int fx = (int)(v % (2 * W)); v /= 2 * W;
    const int fy = (int)(v % (2 * H)); v /= 2 * H;
    const int fz = (int)(v % (2 * D));
    const long n = v / (2 * D);
    const long src = ((n * D + (fz >> 1)) * H + (fy >> 1)) * (long)W + (fx >> 1);
    const long dst = ((n * (2 * D) + fz) * (2 * H) + fy) * (2L * W) + fx;
    *reinterpret_cast<u32x4*>(y + dst * ldy + c) = *reinterpret_cast<const u32x4*>(x + src * ldx + c);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void lp_upsample2_bwd_kernel(const unsigned short* dy, unsigned short* dx, long total8, int D, int H, int W, int C,
                                                               int lddy, int lddx, int accum) {
  const int C8 = C >> 3;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total8; i += (long)gridDim.x * 256) {      // over the COARSE grid
    const int c = (int)(i % C8) * 8;
    long v = i / C8;
    const int ox = (int)(v % W); v /= W;
    const int oy = (int)(v % H); v /= H;
    const int oz = (int)(v % D);
    const long n = v / D;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const long src = (((n * (2 * D) + 2 * oz + (t >> 2)) * (2 * H) + 2 * oy + ((t >> 1) & 1)) * (2L * W) + 2 * ox + (t & 1));
      float f[8];
      unpack8<T>(*reinterpret_cast<const u32x4*>(dy + src * lddy + c), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += f[e];
    }
    const long dst = ((n * D + oz) * H + oy) * (long)W + ox;
    if (accum) {
      float old[8];
      unpack8<T>(*reinterpret_cast<const u32x4*>(dx + dst * lddx + c), old);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += old[e];
    }
    *reinterpret_cast<u32x4*>(dx + dst * lddx + c) = pack8<T>(s);
  }
}
static int lp_sampler_check(int dtype, const void* a, const void* b, int N, int D, int H, int W, int C, int lda, int ldb) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || lda % 8 != 0 || ldb % 8 != 0 || lda < C || ldb < C) return BTS_ERR_SHAPE;
  if ((((uintptr_t)a) & 15) || (((uintptr_t)b) & 15)) return BTS_ERR_ALIGN;
  return BTS_OK;
}
static unsigned lp_sampler_blocks(long total8) { long b = (total8 + 255) / 256; return (unsigned)(b > 16384 ? 16384 : b); }
// (D,H,W) = INPUT dims (even); y (N,D/2,H/2,W/2,C); idx (may be NULL: inference) dense uint8 (N,D/2,H/2,W/2,C)
extern "C" int bts_lp_maxpool2_fwd(int dtype, const void* x, void* y, uint8_t* idx, int N, int D, int H, int W, int C, int ldx, int ldy,
                                   hipStream_t stream) {
  const int r = lp_sampler_check(dtype, x, y, N, D, H, W, C, ldx, ldy);
  if (r != BTS_OK) return r;
  if ((D | H | W) & 1) return BTS_ERR_SHAPE;
  const long total8 = (long)N * (D / 2) * (H / 2) * (W / 2) * (C / 8);
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_maxpool2_fwd_kernel<decltype(t)>, dim3(lp_sampler_blocks(total8)), dim3(256), 0, stream, (const unsigned short*)x, (unsigned short*)y, idx, total8, D / 2, H / 2, W / 2, C, ldx, ldy);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
extern "C" int bts_lp_maxpool2_bwd(int dtype, const void* dy, const uint8_t* idx, void* dx, int N, int D, int H, int W, int C, int lddy, int lddx,
                                   int accumulate, hipStream_t stream) {
  const int r = lp_sampler_check(dtype, dy, dx, N, D, H, W, C, lddy, lddx);
  if (r != BTS_OK) return r;
  if (((D | H | W) & 1) || idx == nullptr) return BTS_ERR_SHAPE;
  const long total8 = (long)N * (D / 2) * (H / 2) * (W / 2) * (C / 8);
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_maxpool2_bwd_kernel<decltype(t)>, dim3(lp_sampler_blocks(total8)), dim3(256), 0, stream, (const unsigned short*)dy, idx, (unsigned short*)dx, total8, D / 2, H / 2, W / 2, C, lddy, lddx, accumulate);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
// (D,H,W) = COARSE dims in both calls
extern "C" int bts_lp_upsample2_fwd(int dtype, const void* x, void* y, int N, int D, int H, int W, int C, int ldx, int ldy, hipStream_t stream) {
  const int r = lp_sampler_check(dtype, x, y, N, D, H, W, C, ldx, ldy);
  if (r != BTS_OK) return r;
  const long total8 = 8L * N * D * H * W * (C / 8);
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_upsample2_fwd_kernel<decltype(t)>, dim3(lp_sampler_blocks(total8)), dim3(256), 0, stream, (const unsigned short*)x, (unsigned short*)y, total8, D, H, W, C, ldx, ldy);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
extern "C" int bts_lp_upsample2_bwd(int dtype, const void* dy, void* dx, int N, int D, int H, int W, int C, int lddy, int lddx, int accumulate,
                                    hipStream_t stream) {
  const int r = lp_sampler_check(dtype, dy, dx, N, D, H, W, C, lddy, lddx);
  if (r != BTS_OK) return r;
  const long total8 = (long)N * D * H * W * (C / 8);
  (void)hipGetLastError();
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_upsample2_bwd_kernel<decltype(t)>, dim3(lp_sampler_blocks(total8)), dim3(256), 0, stream, (const unsigned short*)dy, (unsigned short*)dx, total8, D, H, W, C, lddy, lddx, accumulate);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- output head (decoder.py:55-63): y = sigmoid(x . W + b), 1x1x1 conv to out_ch <= 4 channels, fp32 result (the label map
// is taken from it, so it is never rounded to 16 bits).  One voxel per lane, weights in registers via scalar loads.
template <typename T>
__global__ __launch_bounds__(256) void lp_head_kernel(const unsigned short* x, const float* w, const float* bias, float* y, long nvox, int C,
                                                      int ldx, int K, int sigmoid) {
  for (long v = blockIdx.x * 256L + threadIdx.x; v < nvox; v += (long)gridDim.x * 256) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < C; c0 += 8) {
      float t[8];
      unpack8<T>(*reinterpret_cast<const u32x4*>(x + v * ldx + c0), t);
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < K) acc[k] = fmaf(t[e], w[(c0 + e) * K + k], acc[k]);
    }
    for (int k = 0; k < K; ++k) {
      float o = acc[k] + (bias ? bias[k] : 0.f);
      if (sigmoid) o = 1.f / (1.f + __expf(-o));
      y[v * K + k] = o;
    }
  }
}
// The same with the C/8 lanes of a voxel side by side (C/8 a power of two <= 32): every load instruction of a wave reads 1 KB of
// consecutive bytes (one voxel per lane made each of its four loads touch 64 different lines: 0.65 ms for the 128^3 x 8 head, 2 TB/s);
// the lanes of a voxel add their partial dot products with xor-shuffles, lane 0 of the group writes.
template <typename T, int K>
__global__ __launch_bounds__(256) void lp_head_oct_kernel(const unsigned short* x, const float* w, const float* bias, float* y, long nvox, int C8,
                                                          int ldx, int sigmoid) {
  const int o = threadIdx.x % C8;
  float wr[8][K];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int k = 0; k < K; ++k) wr[e][k] = w[(o * 8 + e) * K + k];
  const long total = nvox * C8;
  const long stride = (long)gridDim.x * 256;
  // (the host launches this kernel with 256 % C8 == 0: a thread's voxel advances by whole steps, no division per 16 bytes)
  const long vpb = 256 / C8, vstride = (long)gridDim.x * vpb;
  long v = blockIdx.x * vpb + threadIdx.x / C8;
  auto one = [&](const u32x4 raw, long vv, bool live) {
    float t[8], acc[K];
    unpack8<T>(raw, t);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(t[e], wr[e][k], s);
      s = lane_group_sum_f32(s, C8);
      acc[k] = s;
    }
    if (live && o == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float r = acc[k] + (bias ? bias[k] : 0.f);
        if (sigmoid) r = 1.f / (1.f + __expf(-r));
        y[vv * K + k] = r;
      }
    }
  };
  // (whole waves stay in the loop: the shuffles need every lane.)  Four steps per trip, their loads issued first.
  for (long i0 = blockIdx.x * 256L; i0 < total; i0 += 4 * stride, v += 4 * vstride) {
    u32x4 raw[4];
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long vv = v + j * vstride;
      live[j] = vv < nvox;
      raw[j] = live[j] ? *reinterpret_cast<const u32x4*>(x + vv * ldx + o * 8) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) one(raw[j], v + j * vstride, live[j]);
  }
}
extern "C" int bts_lp_head(int dtype, const void* x, const float* w, const float* bias, float* y, long nvox, int C, int ldx, int K, int sigmoid,
                           hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (nvox <= 0 || C <= 0 || C % 8 != 0 || K < 1 || K > 4 || ldx % 8 != 0 || ldx < C) return BTS_ERR_SHAPE;
  if (((uintptr_t)x) & 15) return BTS_ERR_ALIGN;
  long blocks = (nvox + 255) / 256;
  if (blocks > 32768) blocks = 32768;
  (void)hipGetLastError();
  const int C8 = C / 8;
  if (C8 >= 2 && C8 <= 32 && (C8 & (C8 - 1)) == 0 && nvox >= 4096) {
    long ob = ((nvox * C8 + 255) / 256 + 3) / 4;      // (four steps per trip of the kernel's loop)
    if (ob > 32768) ob = 32768;
    if (ob < 1) ob = 1;
#define LP_HO(TT, K_) hipLaunchKernelGGL((lp_head_oct_kernel<TT, K_>), dim3((unsigned)ob), dim3(256), 0, stream, (const unsigned short*)x, w, bias, y, nvox, C8, ldx, sigmoid)
#define LP_HO_K(TT) do { if (K == 1) LP_HO(TT, 1); else if (K == 2) LP_HO(TT, 2); else if (K == 3) LP_HO(TT, 3); else LP_HO(TT, 4); } while (0)
    lp_typed(dtype, [&](auto t) { LP_HO_K(decltype(t)); });
#undef LP_HO_K
#undef LP_HO
    BTS_LAUNCH_CHECK();
    return BTS_OK;
  }
  lp_typed(dtype, [&](auto t) {
    hipLaunchKernelGGL(lp_head_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, stream, (const unsigned short*)x, w, bias, y, nvox, C, ldx, K, sigmoid);
  });
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}

// ---- output head backward (decoder.py:55-63 under TF autodiff, train.py:142-151): with dpre = dL/d(x . W + b) per voxel (K <= 4 values,
// the sigmoid's gradient already applied: bts_sigmoid_bwd), ONE pass over the 16-bit activations gives all three gradients:
//   dx[v][c] = sum_k dpre[v][k] W[c][k]  (storage type),   dW[c][k] (+)= sum_v x[v][c] dpre[v][k],   db[k] (+)= sum_v dpre[v][k].
// Round 2 widened x to fp32, ran the fp32 1x1x1 weight- and data-gradient kernels and narrowed dx again: five passes over a 128^3 x 32
// tensor.  One voxel per lane; a lane keeps the C*K + K running sums of its voxels, waves reduce by shuffles, blocks through LDS, one
// fp64 row per block; lp_dbias_finalize_kernel adds the rows in block order.
template <typename T, int C, int K>
__global__ __launch_bounds__(256) void lp_head_bwd_kernel(const unsigned short* x, const float* dpre, const float* w, unsigned short* dx, double* part,
                                                          long nvox, int ldx, int lddx) {
  // lane = (voxel, octet of its C channels): coalesced 16-byte loads / stores; a lane keeps the 8*K sums of its octet (+ K bias sums on
  // octet 0); lanes of equal octet meet by shuffles (stride C/8), waves through LDS, one fp64 row [C*K + K] per block
  constexpr int C8 = C / 8, NS = C * K + K;
  __shared__ float sh[4][NS];
  const int o = threadIdx.x % C8;
  float wr[8][K], acc[8][K], accb[K];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int k = 0; k < K; ++k) { wr[e][k] = w[(o * 8 + e) * K + k]; acc[e][k] = 0.f; }
#pragma unroll
  for (int k = 0; k < K; ++k) accb[k] = 0.f;
  const long total = nvox * C8;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {      // (the stride is a multiple of C8: o is fixed)
    const long v = i / C8;
    float d[K], t[8], ov[8];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = dpre[v * K + k];
    if (o == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) accb[k] += d[k];
    }
    unpack8<T>(*reinterpret_cast<const u32x4*>(x + v * ldx + o * 8), t);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        s = fmaf(d[k], wr[e][k], s);
        acc[e][k] = fmaf(t[e], d[k], acc[e][k]);
      }
      ov[e] = s;
    }
    *reinterpret_cast<u32x4*>(dx + v * lddx + o * 8) = pack8<T>(ov);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float s = acc[e][k];
      for (int m = C8; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
      if (lane < C8) sh[wave][(lane * 8 + e) * K + k] = s;
    }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = accb[k];
    for (int m = C8; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) sh[wave][C * K + k] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NS; i += 256) part[(long)blockIdx.x * NS + i] = ((double)sh[0][i] + (double)sh[1][i]) + ((double)sh[2][i] + (double)sh[3][i]);
}
extern "C" long bts_lp_head_bwd_workspace(int C, int K) { return (C <= 0 || K <= 0) ? -1 : 2048L * (C * K + K) * 8 + 64; }
// x (nvox, C) 16-bit rows of ldx; dpre (nvox, K) fp32 dense; w (C, K) fp32; dx (nvox, C) 16-bit rows of lddx; dw (C, K), db (K) fp32 (+= when accumulate).
// C in {16, 32, 64}, K in {1, 2, 3, 4}: the heads of this model (decoder.py:55-63: C = base_filters, K = out_ch)
extern "C" int bts_lp_head_bwd(int dtype, const void* x, const float* dpre, const float* w, void* dx, float* dw, float* db, void* workspace,
                               long workspace_bytes, long nvox, int C, int ldx, int lddx, int K, int accumulate, hipStream_t stream) {
  if (dtype != LP_F16 && dtype != LP_BF16) return BTS_ERR_UNSUPPORTED;
  if (nvox <= 0 || (C != 16 && C != 32 && C != 64) || K < 1 || K > 4) return BTS_ERR_UNSUPPORTED;
  if (ldx % 8 != 0 || lddx % 8 != 0 || ldx < C || lddx < C) return BTS_ERR_SHAPE;
  if ((((uintptr_t)x) & 15) || (((uintptr_t)dx) & 15) || (((uintptr_t)workspace) & 15)) return BTS_ERR_ALIGN;
  if (workspace_bytes < bts_lp_head_bwd_workspace(C, K)) return BTS_ERR_WORKSPACE;
  long blocks = (nvox * (C / 8) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  double* part = reinterpret_cast<double*>(workspace);
  (void)hipGetLastError();
#define LP_HB(TT, C_, K_) hipLaunchKernelGGL((lp_head_bwd_kernel<TT, C_, K_>), dim3((unsigned)blocks), dim3(256), 0, stream, (const unsigned short*)x, dpre, w, (unsigned short*)dx, part, nvox, ldx, lddx)
#define LP_HB_K(TT, C_) do { if (K == 1) LP_HB(TT, C_, 1); else if (K == 2) LP_HB(TT, C_, 2); else if (K == 3) LP_HB(TT, C_, 3); else LP_HB(TT, C_, 4); } while (0)
#define LP_HB_C(TT) do { if (C == 16) LP_HB_K(TT, 16); else if (C == 32) LP_HB_K(TT, 32); else LP_HB_K(TT, 64); } while (0)
  lp_typed(dtype, [&](auto t) { LP_HB_C(decltype(t)); });
#undef LP_HB_C
#undef LP_HB_K
#undef LP_HB
  BTS_LAUNCH_CHECK();
  const int NS = C * K + K;
  float* tmp = nullptr; (void)tmp;
  // rows -> dw (C*K values) and db (K values): two calls of the fixed-order row adder on the same partial rows
  const int r = bts_lp_dbias_finalize_(part, dw, C * K, (int)blocks, NS, accumulate, stream);
  if (r != BTS_OK || db == nullptr) return r;
  return bts_lp_dbias_finalize_(part + C * K, db, K, (int)blocks, NS, accumulate, stream);
}

// ---- db[c] (+)= the sum of the per-block fp64 partial rows part[b][c] (lp_dbias_block's, the head backward's), one workgroup per column ----
__global__ __launch_bounds__(256) void lp_dbias_finalize_kernel(const double* part, float* db, int nblocks, int C, int accum) {
  __shared__ double sh[4];
  lp_dbias_finalize_body(part, db, nblocks, C, accum, blockIdx.x, sh);
}
int bts_lp_dbias_finalize_(const double* part, float* db, int ncols, int nblocks, int C, int accum, hipStream_t stream) {
  hipLaunchKernelGGL(lp_dbias_finalize_kernel, dim3(ncols), dim3(256), 0, stream, part, db, nblocks, C, accum);
  BTS_LAUNCH_CHECK();
  return BTS_OK;
}
