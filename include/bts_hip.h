/* bts_hip.h -- C ABI of the MI355X (gfx950) 3D U-Net+VAE segmentation engine (libbts_hip.so).
 *
 * Every entry point: plain pointers + sizes, returns int status (0 = ok, >0 = hipError_t, <0 = engine
 * code below), enqueues asynchronously on the caller's hipStream_t, never allocates, never synchronises.
 * Activations are fp32 NDHWC with an explicit pixel stride `ld` (floats between consecutive voxels), so
 * a tensor may be a channel slice of a wider slab (virtual Concatenate).
 * Weights are passed in the reference's Keras layouts and re-packed by bts_conv_pack().
 *
 * What a result may depend on -- the operand views, and nothing else:
 *   - a `workspace` is scratch: its contents on entry are never read before the call has written them, so it need not be initialised
 *     (or cleared between calls); a call that needs zeros there writes them itself;
 *   - an output that is not accumulated into (no BTS_CONV_FLAG_ACCUM / `accumulate` argument set) need not be initialised either: every
 *     element of its view is written, none is read first;
 *   - with ld > C, the ld - C floats between two voxels' channels belong to other tensors of the slab: they are neither written nor do they
 *     influence a result -- a lane outside [0, C) is masked at the load, not loaded and cancelled by a zero weight (Inf * 0 is NaN);
 *   - memory before the first and behind the last voxel of a view is neither read into a result nor written (halo taps outside the
 *     volume are zeros by construction, not loads).
 * The caching allocator of a training process hands out blocks that hold an earlier step's bytes, Inf / NaN after an fp16 overflow step
 * included; tests/test_poison_gpu.py runs every path with such bytes reading NaN and requires bit-identical, finite results.
 *
 * The reference (vliu15/3d-brain-tumor-segmentation) has no FFI of its own: its boundary is the Keras
 * layer protocol. Each function below cites the reference call site whose arithmetic it replaces.
 */
#ifndef BTS_HIP_H
#define BTS_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* bts_stream_t; /* == hipStream_t */

#define BTS_OK 0
#define BTS_ERR_SHAPE (-1)
#define BTS_ERR_ALIGN (-2)
#define BTS_ERR_UNSUPPORTED (-3)
#define BTS_ERR_WORKSPACE (-4)
#define BTS_ERR_RCCL_BASE (-100) /* bts_dp_*: an RCCL call failed; the code is BTS_ERR_RCCL_BASE - ncclResult_t (-101 ncclUnhandledCudaError,
                                    -102 ncclSystemError, -103 ncclInternalError, -104 ncclInvalidArgument, -105 ncclInvalidUsage, ...) */

/* convolution kinds */
#define BTS_CONV_K1 0    /* Conv3D k=1 s=1            layers/resnet.py:30-37, layers/decoder.py:55-63 */
#define BTS_CONV_K3S1 1  /* Conv3D k=3 s=1 'same'     layers/resnet.py:80-87,96-103, layers/vae.py:92-99 */
#define BTS_CONV_K3S2 2  /* Conv3D k=3 s=2 'same'     layers/downsample.py:28-35 (even sizes: pad (0,1)) */
#define BTS_CONV_K3S2T 3 /* Conv3DTranspose k=3 s=2   layers/upsample.py:28-33 (output 2x, tap at 2n cropped) */
#define BTS_ROLE_FWD 0
#define BTS_ROLE_BWD_DATA 1
#define BTS_CONV_FLAG_SIGMOID 1 /* fused activation='sigmoid' (decoder.py:60) */
#define BTS_CONV_FLAG_ACCUM 2   /* add into the destination instead of overwriting */

/* GroupNormalization modes (layers/group_norm.py:83-124) */
#define BTS_GN_SLAB 0    /* channels_last reference semantics: groups = contiguous 1/G chunks of (D,H,W,C) */
#define BTS_GN_CHANNEL 1 /* channels_first reference semantics (true GroupNorm) on NDHWC memory */

/* ---- declarations are appended below, grouped by reference call site ---- */

/* ===== convolutions (layers/resnet.py:30-37,80-87,96-103; downsample.py:28-35; upsample.py:28-33; decoder.py:55-63; vae.py:92-99) ===== */
/* number of floats of the packed weight image for (kind, role); Cin is the slab (folded) input-channel count.
   K3S1 images hold two parts: the implicit-GEMM layout (27 taps) and the Winograd-domain layout (3 x taps x 16 points) */
long bts_conv_packed_floats(int kind, int role, int Cin, int Cout);
/* w: reference Keras layout ((kd,kh,kw,Cin_ref,Cout) or, for K3S2T, (kd,kh,kw,Cout,Cin_ref)); wp: packed image.
 * Cin_slab + dup_shift == Cin_ref. dup_shift>0 folds the encoder's duplicated dense-connection slice
 * (encoder.py:83-87: inputs [o_{j-1}, o_0..o_{j-1}] -> slab [o_0..o_{j-1}], dup_start = (j-1)*F, dup_shift = F). */
int bts_conv_pack(int kind, int role, const float* w, float* wp, int Cin_ref, int Cout, int Cin_slab, int dup_start,
                  int dup_shift, bts_stream_t stream);
/* All weight images in one launch (every image goes stale together at the optimiser step, train.py:152): the caller
 * fills a HOST table of bts_conv_pack_desc_bytes()-sized descriptors with bts_conv_pack_desc (arguments as bts_conv_pack;
 * returns the entry's block count > 0, or a negative engine code; first_block = running sum of those counts), copies it
 * to device memory and passes both copies with the total block count (table_host may be NULL: see below). */
long bts_conv_pack_desc_bytes(void);
long bts_conv_pack_desc(void* host_table, int index, long first_block, int kind, int role, const float* w, float* wp,
                        int Cin_ref, int Cout, int Cin_slab, int dup_start, int dup_shift);
int bts_conv_pack_batch(const void* table_dev, const void* table_host, int n, long total_blocks, bts_stream_t stream);
/* A BTS_CONV_K3S1 image holds three forms of the same weights (implicit GEMM, F(2x2,3x3) x direct, F(2x2x2,3x3x3)); a layer reads the one
 * its geometry selects.  The library records which forms each image has been read in and bts_conv_pack_desc describes those only (all
 * three for an image never read); a form a launch selects although the last re-pack left it out is packed on the spot on the launch's
 * stream.  The counter below grows whenever an image is read in a form it had not been read in before: a host table built at an older
 * value should be rebuilt at the next re-pack (it stays CORRECT either way).  What counts as written is what the table actually RUN
 * wrote: bts_conv_pack_batch reads the forms of each entry from table_host (the host copy the device table was made from), so several
 * tables over one image, or a bts_conv_pack of the whole image between two runs of a narrower cached table, cannot leave a stale form
 * marked fresh.  table_host == NULL: the library cannot tell what the table covers and treats every form of every registered image as
 * stale (correct; each launch then re-packs its form once per weight change).  bts_conv_pack_forget drops the record of an image whose
 * memory is being released (returns 1 if there was one). */
long bts_conv_pack_generation(void);
int bts_conv_pack_forget(const float* wp);
/* y = act(conv(x) + bias). x (N,D,H,W,Cin) stride ldx; y (N,D',H',W',Cout) stride ldy; D' = D | D/2 | 2D. */
/* workspace (may be NULL / 0) lets grids too small to fill the chip split the contraction over workgroups (deterministic
 * two-stage reduction); size from bts_conv3d_fwd_workspace (0 when the shape does not need it). */
long bts_conv3d_fwd_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout);
int bts_conv3d_fwd(int kind, const float* x, const float* wp_fwd, const float* bias, float* y, void* workspace,
                   long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, int flags,
                   bts_stream_t stream);
/* ResNet block pair from one pass over x: y = conv3x3x3(x)+bias (resnet.py:133-134), y2 = conv1x1x1(x)+bias2 (resnet.py:118).
 * wp2 is the BTS_CONV_K1 forward packing. bts_conv3d_fwd_can_fuse() == 0 -> call the two convolutions separately. */
int bts_conv3d_fwd_can_fuse(int N, int D, int H, int W, int Cin, int Cout);
int bts_conv3d_fwd_fused2(const float* x, const float* wp_fwd, const float* bias, float* y, const float* wp2,
                          const float* bias2, float* y2, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy,
                          int ldy2, bts_stream_t stream);
/* dx (+)= conv^T(dy). (D,H,W) are the forward INPUT dims. Replaces tf.GradientTape for these ops (train.py:142-151). */
long bts_conv3d_bwd_data_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout);
int bts_conv3d_bwd_data(int kind, const float* dy, const float* wp_bwd, float* dx, void* workspace, long workspace_bytes,
                        int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy, int flags, bts_stream_t stream);
/* which igemm_kernel<MS,NS,WM,WN,KGS> instantiation a call resolves to (id 0..4, +8 for the 1x1x1 staging variant);
 * used by bench.py to attribute measured launch times to kernel symbols */
int bts_conv3d_fwd_config(int kind, int N, int D, int H, int W, int Cin, int Cout);
int bts_conv3d_bwd_data_config(int kind, int N, int D, int H, int W, int Cin, int Cout);
/* Host only: the profile symbol (bts_profile_get) of the kernel that takes a call first -- 20 merged transposed | 21 streaming 1x1x1 |
 * 22 direct <= 4 couts | 25 two-channel input | 23 Winograd F(2x2,3x3) x direct | 27 Winograd F(2x2x2,3x3x3) | the tiled kernel's
 * bts_conv3d_*_config id -- or the negative status of a call no kernel takes.  dir 0: bts_conv3d_fwd's kind, sizes, ldx, ldy and flags;
 * dir 1: bts_conv3d_bwd_data's (ldx = lddx, ldy = lddy).  second: 0 | 1 the fused shortcut output of bts_conv3d_fwd_fused2 (ld2 = ldy2) |
 * 2 the second input of bts_conv3d_bwd_data_pair (ld2 = lddy2), both BTS_CONV_K3S1 only.  G > 0: GroupNorm partials asked for
 * (bts_conv3d_fwd_gn).  aligned: bit 0 the tensor read, 1 the tensor written, 2 y2 | dy2, 3 the workspace lies on a 16-byte boundary.
 * workspace_bytes: what the call may use, 0 none, < 0 as much as it asks for.  The BTS_WINO, BTS_W3, BTS_WINO_MIN_WGS, BTS_IGEMM_*
 * environment switches are read per call, as the launches read them. */
int bts_conv3d_kernel(int dir, int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, int flags, int second,
                      int ld2, int G, int aligned, long workspace_bytes);
/* Host only: the convolution launches bts_conv3d_bwd_data_pair makes for the described call -- 1: one kernel forms both terms (the
 * tiled kernel, or the Winograd F(2x2x2,3x3x3) kernel with the 1x1x1 term in its output side), 2: the 1x1x1 term is a launch of its
 * own (two calls, or a Winograd kernel that leaves it over) -- or the negative status of a call no kernel takes.  Sizes, strides and
 * flags as bts_conv3d_bwd_data_pair's.  aligned: bit 0 dy, 1 dx, 2 dy2, 3 the workspace lies on a 16-byte boundary.  workspace_bytes:
 * what the call may use, 0 none, < 0 as much as it asks for.  The environment switches are read per call, as the launch reads them. */
int bts_conv3d_bwd_data_pair_launches(int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy, int lddy2, int flags,
                                      int aligned, long workspace_bytes);
long bts_conv3d_bwd_weight_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout);
/* dw in the reference layout (Cin_ref = Cin + dup_shift); db (may be NULL; not produced for K3S2T: use bts_colsum). */
int bts_conv3d_bwd_weight(int kind, const float* x, const float* dy, float* dw, float* db, void* workspace,
                          long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy,
                          int dup_start, int dup_shift, int accumulate, bts_stream_t stream);
/* Host only: the profile symbol (bts_profile_get) of the kernel bts_conv3d_bwd_weight runs for the described call -- the direct kernel
 * with 100 register staging | 104 LDS-DMA staging | 109, 110 the fixed-geometry sweeps of stride 1, 2; 24 Winograd F(2x2x2,3x3x3)
 * (wgw_kernel); 26 the streaming 1x1x1 kernel (k1w_kernel) -- or the negative status of a call it does not take.  The counterpart of
 * bts_conv3d_kernel: the launch, this query, bts_conv3d_bwd_weight_form and bts_conv3d_bwd_weight_workspace answer from one choice.
 * Sizes and strides as bts_conv3d_bwd_weight's.  aligned: bit 0 x, bit 1 dy lies on a 16-byte boundary.  The BTS_WGW and BTS_K1W
 * environment switches are read per call, as the launch reads them. */
int bts_conv3d_bwd_weight_kernel(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned);
/* Host only: the form of that kernel -- 3 Winograd F(2x2x2,3x3x3) where it is 24, 0 for every other (the direct kernels and the
 * streaming 1x1x1 kernel, which bts_conv3d_bwd_weight_kernel tells apart) -- or the negative status. */
int bts_conv3d_bwd_weight_form(int kind, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int aligned);

/* ===== GroupNormalization (layers/group_norm.py:83-124) ===== */
/* Statuses, all before any launch: BTS_ERR_SHAPE for a non-positive size, C < G or G not dividing C (the queries return -1);
 * BTS_ERR_ALIGN for ldy / lddy < C and, on a vectorisable shape (C a power of two in [4, 1024], group length a multiple of 4, row
 * stride a multiple of 4), for x, y, dy or dx off a 16-byte boundary; BTS_ERR_WORKSPACE for a NULL or short workspace. */
long bts_gn_workspace(int N, long V, int C, int G, int mode);
long bts_gn_bwd_workspace(int N, long V, int C, int G, int mode);
/* mean,rstd: (N*G) floats. x dense NDHWC (ld == C). */
int bts_gn_stats(const float* x, float* mean, float* rstd, void* workspace, long workspace_bytes, int N, long V, int C,
                 int G, int mode, float eps, bts_stream_t stream);
/* y = [relu](gamma_b*(x-mean)*rstd + beta_b); y may be a channel slice (ldy >= C). */
int bts_gn_apply(const float* x, float* y, const float* gamma, const float* beta, const float* mean, const float* rstd,
                 int N, long V, int C, int ldy, int G, int mode, int relu, bts_stream_t stream);
int bts_gn_bwd(const float* x, const float* dy, float* dx, const float* gamma, const float* beta, const float* mean,
               const float* rstd, float* dgamma, float* dbeta, void* workspace, long workspace_bytes, int N, long V, int C,
               int lddy, int G, int mode, int relu, int accumulate_params, bts_stream_t stream);

/* ===== squeeze-excitation gate + block epilogue (layers/resnet.py:116-138) ===== */
long bts_colsum_workspace(int N, long rows, int C);
int bts_colsum(const float* x, float* out, void* workspace, long workspace_bytes, int N, long rows, int C, int ld,
               float scale, int sum_over_n, int accumulate, bts_stream_t stream);
int bts_se_mlp_fwd(const float* gap, const float* w1, const float* w2, float* h, float* ch, int N, int F, int R,
                   bts_stream_t stream);
/* out = res*(sigmoid(res.wsp)+ch) + relu(GN2(c2)); c2 may be NULL (gate only). sp: (N*V) saved for backward. */
int bts_block_epilogue_fwd(const float* res, const float* c2, float* out, float* sp, const float* wsp, const float* ch,
                           const float* gamma, const float* beta, const float* mean, const float* rstd, int N, long V,
                           int F, int ldo, int G, int mode, bts_stream_t stream);
/* F a power of two in [4, 256] and lddo >= F a multiple of 4, N, V, R positive: BTS_ERR_SHAPE otherwise (the query returns -1);
 * BTS_ERR_WORKSPACE for a NULL or short workspace, BTS_ERR_ALIGN for one off a 16-byte boundary; all before any launch.
 * bts_block_epilogue_fwd: BTS_ERR_SHAPE for the same F rule, ldo < F, ldo % 4 != 0 or (with c2) G not dividing F; BTS_ERR_ALIGN for
 * res, out or c2 off a 16-byte boundary. */
long bts_se_bwd_workspace(int N, long V, int F, int R);
int bts_se_bwd(const float* dout, const float* res, const float* sp, const float* gap, const float* h, const float* ch,
               const float* w1, const float* w2, const float* wsp, float* dres, float* ds, float* dgap, float* dw1,
               float* dw2, float* dwsp, void* workspace, long workspace_bytes, int N, long V, int F, int R, int lddo,
               int accumulate_params, bts_stream_t stream);

/* A ResnetBlock's gate backward (bts_se_bwd) and GroupNorm-2 backward (bts_gn_bwd, slab mode, ReLU) in one pair of passes: what
 * tf.GradientTape (train.py:142,151) derives for layers/resnet.py:121-137 from the gradient of the block output.  dout (N,V,F) rows of
 * lddo floats; res, c2 dense; outputs dres, dc2 dense, ds (N*V) and dgap (N,F) scratch.  accumulate_*: += into the parameter gradients.
 * The workspace query returns -1 and the call BTS_ERR_UNSUPPORTED outside the kernels' tiling (the caller runs the two separate calls). */
long bts_block_bwd_workspace(int N, long V, int F, int R, int G);
int bts_block_bwd(const float* dout, int lddo, const float* res, const float* c2, const float* sp, const float* gap, const float* h,
                  const float* ch, const float* w1, const float* w2, const float* wsp, const float* gamma, const float* beta,
                  const float* mean, const float* rstd, float* dres, float* dc2, float* ds, float* dgap, float* dw1, float* dw2,
                  float* dwsp, float* dgamma, float* dbeta, void* workspace, long workspace_bytes, int N, long V, int F, int R, int G,
                  int accumulate_gate_params, int accumulate_norm_params, bts_stream_t stream);

/* ===== element-wise (layers/encoder.py:39,71; layers/vae.py:9-13) ===== */
int bts_dropout_mask(uint8_t* mask, long n, float rate, uint64_t seed, bts_stream_t stream);
int bts_dropout_apply(const float* x, const uint8_t* mask, float* y, long n, float rate, bts_stream_t stream);
int bts_normal(float* out, long n, uint64_t seed, bts_stream_t stream);
int bts_vae_sample_fwd(const float* proj, const float* eps, float* z, int N, int L, bts_stream_t stream);
/* dproj (N, 2L) += the gradient of z: dproj[:, :L] += dz, dproj[:, L:] += dz * 0.5 * exp(0.5 * logvar) * eps.  ACCUMULATES: dproj already
 * holds the loss's own gradient with respect to proj (bts_loss_bwd) when the tape reaches the sampling step. */
int bts_vae_sample_bwd(const float* proj, const float* eps, const float* dz, float* dproj, int N, int L, bts_stream_t stream);
int bts_fill(float* p, long n, float v, bts_stream_t stream);
int bts_axpy(float* y, const float* x, long n, float a, bts_stream_t stream);
int bts_add_strided(float* dst, const float* src, long rows, int C, int ldd, int lds_, int accumulate, bts_stream_t stream);
int bts_scalar_lincomb(float* out, const float* a, const float* b, float ca, float cb, bts_stream_t stream);
int bts_relu_bwd(const float* y, const float* dy, float* dx, long n, bts_stream_t stream);
/* dx (rows,C dense) = dy*y*(1-y): gradient through the fused output sigmoid (decoder.py:60) */
int bts_sigmoid_bwd(const float* y, const float* dy, float* dx, long rows, int C, int ldy, int lddy, bts_stream_t stream);

/* ===== Dense (layers/vae.py:61-64,105-109) ===== */
long bts_dense_workspace(int N, int in, int out);
int bts_dense_fwd(const float* x, const float* w, const float* bias, float* y, void* workspace, long workspace_bytes, int N,
                  int in, int out, int relu, bts_stream_t stream);
int bts_dense_bwd(const float* x, const float* w, const float* g, float* dx, float* dw, float* db, int N, int in, int out,
                  int accumulate_dx, int accumulate_params, bts_stream_t stream);

/* ===== loss / metric / regulariser (util.py:13-24,35-57; train.py:146) ===== */
long bts_loss_workspace(void);
/* sums: 3C+4 doubles = I[C],P[C],T[C], sum (x-y_vae)^2, KL sum, numel_x, numel_z -- all-reduce these for data parallel */
int bts_loss_sums(const float* y_pred, const float* y, const float* x, const float* y_vae, const float* proj, double* sums,
                  void* workspace, long workspace_bytes, int N, long V, int C, int ldp, int ldy, int Cx, int ldx, int ldv,
                  int Lz, bts_stream_t stream);
int bts_loss_value(const double* sums, float* loss, float* parts, int C, int has_vae, bts_stream_t stream);
/* dlogit (N,V,C) and dyvae (N,V,Cx) are written DENSE (voxel strides C and Cx) whatever ldp / ldy / ldx / ldv say about the inputs; dproj
 * (N, 2 Lz) is overwritten.  gscale: one device float or NULL (= 1).  through_sigmoid: multiply by p (1 - p) of the given y_pred. */
int bts_loss_bwd(const float* y_pred, const float* y, const float* x, const float* y_vae, const float* proj,
                 const double* sums, const float* gscale, float* dlogit, float* dyvae, float* dproj, int N, long V, int C,
                 int ldp, int ldy, int Cx, int ldx, int ldv, int Lz, int through_sigmoid, bts_stream_t stream);
/* Compound loss (no reference counterpart): loss = w_dice * dice + w_ce * CE + 0.1 * l2 + 0.1 * kl with dice, l2, kl as above and
 * CE = sum(e) / (N_global V C), e = w_pos t (1-q)^gamma (-log q) + w_neg (1-t) q^gamma (-log(1-q)), q = min(max(p, 2^-23), 1 - 2^-23):
 * gamma = 0 is binary cross-entropy, gamma > 0 the focal loss, alpha is w_pos = alpha, w_neg = 1 - alpha.  Each entry point makes ONE pass.
 * sums: 4C+5 doubles = the 3C+4 of bts_loss_sums, sum e per channel [C], this shard's N*V -- raw sums, all-reduce them for data parallel.
 * parts[4] = dice, l2, kl, CE.  dlogit = w_dice * (the Dice gradient) + w_ce / (sums[4C+4] * C) * d sum(e), times *gscale; d e / d p is the
 * clamped formula's (zero where p < 2^-23 or p > 1 - 2^-23); dyvae, dproj and the dense outputs as bts_loss_bwd.  BTS_ERR_SHAPE for C outside
 * 1..8, N, V <= 0 or a voxel stride below its channel count; BTS_ERR_UNSUPPORTED for gamma outside [0, 8] or a negative / non-finite
 * weight; BTS_ERR_WORKSPACE below bts_seg_loss_workspace() bytes. */
long bts_seg_loss_workspace(void);
int bts_seg_loss_sums(const float* y_pred, const float* y, const float* x, const float* y_vae, const float* proj, double* sums,
                      void* workspace, long workspace_bytes, int N, long V, int C, int ldp, int ldy, int Cx, int ldx, int ldv,
                      int Lz, float gamma, float w_pos, float w_neg, bts_stream_t stream);
int bts_seg_loss_value(const double* sums, float* loss, float* parts, int C, int has_vae, float w_dice, float w_ce,
                       bts_stream_t stream);
int bts_seg_loss_bwd(const float* y_pred, const float* y, const float* x, const float* y_vae, const float* proj,
                     const double* sums, const float* gscale, float* dlogit, float* dyvae, float* dproj, int N, long V, int C,
                     int ldp, int ldy, int Cx, int ldx, int ldv, int Lz, int through_sigmoid, float w_dice, float w_ce, float gamma,
                     float w_pos, float w_neg, bts_stream_t stream);
/* table: (cells*C*3) doubles, cells = W if channels_last_axes else 1; labels: (N*V) uint8 or NULL */
int bts_dice_metric_sums(const float* y_true, const float* y_pred, uint8_t* labels, double* table, int N, long V, int W,
                         int C, int ldt, int ldp, int channels_last_axes, bts_stream_t stream);
int bts_dice_metric_value(const double* table, float* out, int W, int C, int channels_last_axes, bts_stream_t stream);
long bts_l2_workspace(void);
int bts_l2_reg_fwd(const float* params, const long* off, const long* len, const float* coef, int nranges, float* out,
                   void* workspace, long workspace_bytes, bts_stream_t stream);
int bts_l2_reg_bwd(const float* params, float* grads, const long* off, const long* len, const float* coef, int nranges,
                   const float* gscale, bts_stream_t stream);

/* ===== optimiser (util.py:60-84; Keras Adam, epsilon un-corrected) ===== */
int bts_adam_tf_step(float* p, const float* g, float* m, float* v, long n, float lr_t, float beta1, float beta2, float eps,
                     float gmul, bts_stream_t stream);
/* Dynamic loss scaling of the fp16-storage trainer without a host round trip (no reference counterpart: the reference trains in
 * fp32, train.py:140-152): flag[0] = 1 iff any gradient element is Inf / NaN; the guarded step is bts_adam_tf_step unless *skip != 0,
 * in which case nothing is written (the step is skipped on the device; the host learns of it one step later). */
int bts_grad_nonfinite(const float* g, long n, int* flag, bts_stream_t stream);
int bts_adam_tf_step_guarded(float* p, const float* g, float* m, float* v, long n, float lr_t, float beta1, float beta2, float eps,
                             float gmul, const int* skip, bts_stream_t stream);

/* ===== the two data-gradient paths into a ResNet block's input in one pass (resnet.py:118,134: x feeds conv1 and the
 * 1x1x1 shortcut) ===== */
/* dx (+)= bwd_data(3x3x3 s1)(dy, wp_bwd) + bwd_data(1x1x1)(dy2, wp2_bwd); both weight images in BTS_ROLE_BWD_DATA packing.
 * The 1x1x1 term is evaluated at the centre tap of the 3x3x3 sweep; the library falls back to two launches where that is
 * not possible (split-K grids, unaligned dy2). */
long bts_conv3d_bwd_data_pair_workspace(int N, int D, int H, int W, int Cin, int Cout);
int bts_conv3d_bwd_data_pair(const float* dy, const float* wp_bwd, const float* dy2, const float* wp2_bwd, float* dx,
                             void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int lddx, int Cout,
                             int lddy, int lddy2, int flags, bts_stream_t stream);

/* ===== convolution + GroupNorm statistics of its output in one pass (resnet.py:80-93: conv -> GroupNormalization) ===== */
/* y = conv(x) + bias, y DENSE (voxel stride Cout), and (mean, rstd)[N*G] = BTS_GN_SLAB statistics of y.  The sums come out of
 * the conv epilogue when the tiled kernel takes the launch (no split-K, whole tiles per z-slab group); otherwise the library
 * runs bts_gn_stats on y itself.  Workspace (required) from bts_conv3d_fwd_gn_workspace. */
long bts_conv3d_fwd_gn_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout, int G);
int bts_conv3d_fwd_gn(int kind, const float* x, const float* wp_fwd, const float* bias, float* y, void* workspace,
                      long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int G, float eps, float* mean,
                      float* rstd, bts_stream_t stream);
/* the fused shortcut pair (bts_conv3d_fwd_fused2) with the statistics of its 3x3x3 output y */
int bts_conv3d_fwd_fused2_gn(const float* x, const float* wp_fwd, const float* bias, float* y, const float* wp2,
                             const float* bias2, float* y2, void* workspace, long workspace_bytes, int N, int D, int H, int W,
                             int Cin, int ldx, int Cout, int ldy2, int G, float eps, float* mean, float* rstd,
                             bts_stream_t stream);

/* ===== non-default samplers (downsample.py:51-70, upsample.py:49-79) ===== */
/* MaxPooling3D(pool 2, stride 2) on even (D,H,W): y (N,D/2,H/2,W/2,C); idx (dense, one byte per output element) records the
 * window position dz*4+dy*2+dx of the first maximum and routes the gradient in bts_maxpool2_bwd (D,H,W = INPUT dims). */
int bts_maxpool2_fwd(const float* x, float* y, uint8_t* idx, int N, int D, int H, int W, int C, int ldx, int ldy,
                     bts_stream_t stream);
int bts_maxpool2_bwd(const float* dy, const uint8_t* idx, float* dx, int N, int D, int H, int W, int C, int lddy, int lddx,
                     int accumulate, bts_stream_t stream);
/* UpSampling3D(size 2) = nearest-neighbour repeat: y (N,2D,2H,2W,C) from x (N,D,H,W,C); backward sums the 8 children
 * (D,H,W = COARSE dims in both calls). */
int bts_upsample2_fwd(const float* x, float* y, int N, int D, int H, int W, int C, int ldx, int ldy, bts_stream_t stream);
int bts_upsample2_bwd(const float* dy, float* dx, int N, int D, int H, int W, int C, int lddy, int lddx, int accumulate,
                      bts_stream_t stream);

/* ===== full-volume inference helpers (test.py:95-151,259-261) ===== */
/* dst (+)= scale * t(flip(src)) on dense NDHWC tensors; flip_mask bits 4|2|1 reverse D|H|W (tf.reverse, test.py:139,142);
 * mean/stdv (C floats, both or neither): t(v) = (v - mean[c]) / std[c] (test.py:111), identity when NULL. src != dst
 * unless flip_mask == 0. */
int bts_flip_affine(const float* src, float* dst, const float* mean, const float* stdv, int N, int D, int H, int W, int C,
                    int flip_mask, float scale, int accumulate, bts_stream_t stream);
/* y = prob * bmask (test.py:154-155; bmask one float per voxel) and/or the label map the script intends: argmax_c + 1,
 * values >= 3 -> 4 (test.py:259-261), 0 where masked out or below `threshold`.  y and labels may each be NULL. */
int bts_tta_finish(const float* prob, const float* bmask, float* y, uint8_t* labels, long nvox, int C, float threshold,
                   bts_stream_t stream);

/* ===== resampling of a scan to the 1 mm^3 grid and back (test.py:15-72: Interpolator, scipy.ndimage.zoom(order=3, mode='reflect')) =====
 * Dense fp32 (D,H,W,C) tensors, C innermost, 1 <= C <= 8; every channel is resampled on its own (zoom() per channel on 3-D arrays). */
/* cubic B-spline coefficients of src along D, H and W with the exact half-sample-symmetric ('reflect') boundary (the spline_filter
 * half of zoom(), test.py:46,62); src == dst allowed; spatial extents < 4 return BTS_ERR_SHAPE. */
int bts_spline_prefilter3d(const float* src, float* dst, int D, int H, int W, int C, bts_stream_t stream);
/* dst (Dpad,Hpad,Wpad,C) = coef (Din,Hin,Win,C) evaluated on the (Dout,Hout,Wout) grid of zoom(): output index o reads input
 * coordinate o * (n-1)/(nout-1); order 0 | 1 | 3 (3: coef from bts_spline_prefilter3d; 0, 1: the samples themselves), reflect
 * index mapping (test.py:46,62).  bmask (Dpad,Hpad,Wpad; may be NULL) = max_c value > 0 (test.py:53-54).  Voxels outside
 * (Dout,Hout,Wout) are written as zero in both outputs (pad_to_spatial_res, test.py:164-178, without a pass of its own).
 * mean/stdv (C floats, both or neither): dst = (value - mean[c]) / std[c] (test.py:107) applied after the mask test to every
 * voxel, the padding included, i.e. dst is the normalised padded volume. */
int bts_zoom3d(const float* coef, float* dst, float* bmask, const float* mean, const float* stdv, int Din, int Hin, int Win,
               int Dout, int Hout, int Wout, int C, int Dpad, int Hpad, int Wpad, int order, bts_stream_t stream);

/* ===== conforming a scan to an oriented grid by its affine (infer.Conformer; the reference stacks its modalities voxel for voxel,
 * test.py:21-42, whatever their headers say) =====
 * Dense fp32 (D,H,W,C) tensors, C innermost, 1 <= C <= 8. */
/* dst = the exact copy flip(transpose(src)): src is (D,H,W,C); output axis a runs along source axis perm_a (a permutation of 0, 1, 2), so
 * dst is (S[perm0],S[perm1],S[perm2],C) with S = (D,H,W); flip_mask bits 4|2|1 reverse OUTPUT axis 0|1|2.  numpy:
 * np.flip(np.transpose(src, (perm0, perm1, perm2, 3)), the flipped axes).  src and dst must not overlap.  BTS_ERR_SHAPE for a bad extent,
 * permutation or mask, a NULL pointer or src == dst, BTS_ERR_ALIGN for a volume that does not start on a voxel's vector width (16 bytes
 * for C % 4 == 0, 8 for C == 2), with nothing launched. */
int bts_reorient3d(const float* src, float* dst, int D, int H, int W, int C, int perm0, int perm1, int perm2, int flip_mask,
                   bts_stream_t stream);
/* dst[o0,o1,o2, c0 .. c0+C-1] = coef (Ds,Hs,Ws,C) evaluated at the source voxel coordinate s = m12 (o0,o1,o2,1), m12 a HOST array of 12
 * doubles (3 x 4, row-major) read during the call; s is formed in fp64.  dst is (Dp,Hp,Wp,ld_dst), ld_dst >= c0 + C; its other channels
 * are not touched.  order 0 | 1 | 3 with the taps and reflect index mapping of bts_zoom3d (3: coef from bts_spline_prefilter3d, its
 * fp32 weights and summation order; 1: the 8 taps weighted and summed in fp64 and rounded once).  An output voxel whose s lies outside [-0.5, n - 0.5] on any axis is 0, as are the voxels outside (Do,Ho,Wo).
 * bmask (Dp,Hp,Wp; may be NULL) = max_c value > 0, only for a call that writes every channel (c0 == 0 and ld_dst == C).
 * BTS_ERR_SHAPE for a bad extent, ld_dst < C, a channel range outside ld_dst, a NULL coef, dst or m12, or a bmask with other channels
 * present, with nothing launched. */
int bts_affine_resample3d(const float* coef, int Ds, int Hs, int Ws, int C, float* dst, int ld_dst, int c0, float* bmask, int Do, int Ho,
                          int Wo, int Dp, int Hp, int Wp, const double* m12, int order, bts_stream_t stream);
/* A label map through a general affine (python -m bts_amd.preprocess --conform): lab is a dense fp32 (Ds,Hs,Ws) volume of label values
 * (any finite values), dst a dense fp32 (Dp,Hp,Wp) one.  Per output voxel inside (Do,Ho,Wo): s = m12 (o0,o1,o2,1) as
 * bts_affine_resample3d forms it; 0 where s lies outside [-0.5, n - 0.5] on any axis or is not finite; else the 8 taps of order 1
 * (floor(s), floor(s) + 1 per axis, reflected; fp64 weights (wd * wh) * ww, row-major tap order) vote: a value's weight is the sum, in
 * tap order, of the weights of the taps that hold it, the value with the largest weight wins and, of exactly equal weights, the smallest
 * value.  This is the arg-max over classes of each class indicator interpolated linearly, in one gather, for any set of values.  The
 * voxels outside (Do,Ho,Wo) are 0.  No atomics, no workspace: deterministic.  BTS_ERR_SHAPE for an extent < 1, Dp < Do (and so on), a
 * NULL lab, dst or m12, or lab == dst; BTS_ERR_ALIGN for a pointer off a float's alignment; with nothing launched. */
int bts_label_resample3d(const float* lab, int Ds, int Hs, int Ws, float* dst, int Do, int Ho, int Wo, int Dp, int Hp, int Wp,
                         const double* m12, bts_stream_t stream);

/* ===== segmenting a folder of scans end to end (test.py:181-270: main) =====
 * The skull-stripping hand-over between the two models (test.py:244-254: invert, multiply, slice, pad again) in one pass.
 * x (Da,Ha,Wa,C) fp32: the scan padded to the skull model's resolution; p (Da,Ha,Wa,1): that stage's masked mean probability; m
 * (Da,Ha,Wa,1): the brain mask.  (D,H,W): the unpadded extent; (Db,Hb,Wb): the tumour model's padded extent, each axis >= (D,H,W).
 * xo (Db,Hb,Wb,C) = x * (1.0f - p) inside (D,H,W), 0 outside; mo (Db,Hb,Wb,1) = m inside, 0 outside (the mask is carried unchanged,
 * test.py:251-254).  One fp32 subtract and one fp32 multiply per value: bit-equal to numpy float32 x * (1 - p).  BTS_ERR_SHAPE for
 * C < 1, a non-positive extent, or an unpadded extent larger than either padded one. */
int bts_skull_strip(const float* x, const float* p, const float* m, float* xo, float* mo, int Da, int Ha, int Wa, int D, int H, int W,
                    int Db, int Hb, int Wb, int C, bts_stream_t stream);
/* The device side of the per-case score (test.py:226-232,266-270; the Dice sums of util.py:50-55 follow from the counts on the host):
 * counts[min(t,K-1) * K + min(p,K-1)] += 1 for every voxel of two dense uint8 label maps (truth, prediction), K in 2..8; counts: K*K
 * int64 on the device, accumulated across calls (zero it once per score).  K = 4 folds BraTS label 4 onto class 3 (preprocess.py:36).
 * Integer atomics only: exact and bit-reproducible.  BTS_ERR_SHAPE for K outside 2..8 or nvox < 0; nvox == 0 launches nothing. */
int bts_label_confusion(const uint8_t* truth, const uint8_t* pred, long nvox, int K, long* counts, bts_stream_t stream);
/* The distance side of the per-case score (test.py:266-270): the 95th-percentile Hausdorff distance of a region is taken from the three
 * calls below and a few float64 operations on the host (bts_amd.infer.surface_scores).
 * Surface of one region of a dense uint8 label map (D,H,W): a voxel belongs to the region when bit min(label, K-1) of class_mask is set
 * (K in 2..8, 0 <= class_mask < 2^K; WT = 14, TC = 10, ET = 8 for K = 4), and is a surface voxel when one of its six face neighbours is
 * outside the region or outside the volume.  surf (uint8, every byte written) = 1 on surface voxels, 0 elsewhere; *count (int64 on the
 * device, accumulated across calls) += their number.  BTS_ERR_SHAPE for a non-positive extent, K outside 2..8 or a class_mask outside
 * its range. */
int bts_region_surface(const uint8_t* lab, uint8_t* surf, long* count, int D, int H, int W, int K, int class_mask, bts_stream_t stream);
/* dist2 (D,H,W) float64 = squared distance in mm^2 from each voxel to the nearest voxel with feat != 0 on a grid of spacing (sd,sh,sw)
 * mm; +inf everywhere when there is none (test.py:266-270).  Exact and separable: along W, then H, then D, out[i] = min over all j of the
 * line of g[j] + (s (i - j)) (s (i - j)), each product and the sum rounded once; the H and D passes run in place.  BTS_ERR_SHAPE for a
 * non-positive extent, an extent above 8192 (a line is staged in LDS) or a spacing that is not positive and finite. */
int bts_edt3d_sq(const uint8_t* feat, double* dist2, int D, int H, int W, double sd, double sh, double sw, bts_stream_t stream);
/* Exact order statistics for the percentile of the score (test.py:266-270): out[i] = the ranks[i]-th smallest (0-based) of
 * {v[j] : mask[j] != 0, j < n}, nan where ranks[i] is not below the number of selected values.  v: NON-NEGATIVE float64 (they order as
 * their bit patterns; +inf allowed), mask: uint8, ranks: nranks <= 8 HOST values, out: nranks device doubles, work: device memory of
 * bts_masked_select_workspace(nranks) bytes.  Radix select, 8 passes of an integer histogram and a one-workgroup pick, no host round
 * trip: the bits of a sort, the same in every run.  BTS_ERR_SHAPE for n < 0, nranks outside 0..8 or a negative rank; n == 0 or
 * nranks == 0 launches nothing and leaves out untouched. */
long bts_masked_select_workspace(int nranks);
int bts_masked_select(const double* v, const uint8_t* mask, long n, const long* ranks, int nranks, double* out, void* work,
                      bts_stream_t stream);
/* Connected components for cleaning a label map before it is written and scored (the arg-max of test.py:259-261 is used as it is by the
 * reference; bts_amd.infer.remove_components, postprocess_labels).  The region is that of bts_region_surface: bit min(label, K-1) of
 * class_mask; connectivity 6, 18 or 26 = scipy's generate_binary_structure(3, 1|2|3).  comp (int32 (D,H,W), every element written) = 0
 * outside the region and 1 + the smallest linear index (d H + h) W + w of the voxel's component inside: a function of the input alone,
 * the same bytes in every run; comp[v] == v + 1 marks a component's root.  Union-find on the device: tiles in LDS, then the tile seams
 * with agent-scope integer atomicMin, then a flattening pass.  BTS_ERR_SHAPE for a non-positive extent, D H W >= 2^31 - 1, K outside
 * 2..8, a class_mask outside its range or a connectivity other than 6, 18, 26. */
int bts_components3d(const uint8_t* lab, int* comp, int D, int H, int W, int K, int class_mask, int connectivity, bts_stream_t stream);
/* size (n int32, zeroed by the call): size[r] = the number of voxels whose root is r (comp == r + 1); *ncomp (int64 on the device,
 * accumulated across calls) += the number of components.  BTS_ERR_SHAPE for n < 0 or n >= 2^31 - 1; n == 0 launches nothing. */
int bts_component_sizes(const int* comp, long n, int* size, long* ncomp, bts_stream_t stream);
/* *key (one 64-bit word on the device, zeroed by the call) = max over the components of (size << 32) | (0xFFFFFFFF - root): the largest
 * component, the smallest root among equal sizes; 0 when there is none.  Same guards as bts_component_sizes. */
int bts_component_largest(const int* size, long n, uint64_t* key, bts_stream_t stream);
/* In place on the uint8 map: every voxel with comp != 0 whose component fails `size[root] >= min_voxels and (not largest_only or root ==
 * the root of *key)` becomes `fill`, and *removed_voxels (int64 on the device, accumulated) += 1; *removed_components (may be NULL) += 1
 * per failing component.  No other voxel is written.  key may be NULL unless largest_only.  BTS_ERR_SHAPE for n outside [0, 2^31 - 1),
 * min_voxels < 0, fill outside 0..255 or largest_only without a key; n == 0 launches nothing. */
int bts_components_apply(uint8_t* lab, const int* comp, const int* size, const uint64_t* key, long n, int min_voxels, int largest_only,
                         int fill, long* removed_voxels, long* removed_components, bts_stream_t stream);
/* In place: when the region (K, class_mask as above) holds between 1 and limit - 1 voxels, each of them becomes `fill` and *changed
 * (int64 on the device, accumulated) += their number; the BraTS convention for a tiny enhancing region.  confusion: the K x K int64
 * counts of bts_label_confusion(lab, lab) on the device, whose diagonal holds the class sizes, so the decision takes no host round trip.
 * BTS_ERR_SHAPE for n < 0, K outside 2..8, a class_mask outside its range, fill outside 0..255 or limit < 0; n == 0 or limit == 0
 * launches nothing. */
int bts_region_relabel(uint8_t* lab, long n, int K, int class_mask, int fill, const long* confusion, long limit, long* changed,
                       bts_stream_t stream);
/* Lesion-wise scores (the BraTS 2023 ranking; bts_amd.infer.lesionwise_scores): what lies between the labelling above and the distances
 * of bts_region_surface / bts_edt3d_sq / bts_masked_select.  Regions (K, class_mask) and connectivities are those of bts_components3d.
 * out (uint8 (D,H,W), every byte written, must not overlap lab) = 1 where scipy.ndimage.binary_dilation(region,
 * generate_binary_structure(3, 1|2|3), iterations, border_value=0) is set, 0 elsewhere; iterations == 0 gives the region itself.  A tiled
 * stencil on bit rows in LDS; a pass runs `fuse` iterations on a tile with a halo of as many voxels (0: the default, 3; at most 6) and
 * ceil(iterations / fuse) passes alternate between out and work, device memory of bts_dilate3d_workspace(...) bytes (0 for one pass; work
 * may then be NULL).  BTS_ERR_SHAPE, before any HIP call, for a non-positive extent, D H W >= 2^31 - 1, iterations outside 0..4096, fuse
 * outside 0..6, K outside 2..8, a class_mask outside its range or a connectivity other than 6, 18, 26; BTS_ERR_WORKSPACE for a missing
 * workspace. */
long bts_dilate3d_workspace(int D, int H, int W, int iterations, int fuse);
int bts_dilate3d(const uint8_t* lab, uint8_t* out, int D, int H, int W, int K, int class_mask, int connectivity, int iterations, int fuse,
                 void* work, bts_stream_t stream);
/* One pass over n voxels of td_comp (bts_components3d of the dilated truth), truth (uint8, region K / class_mask) and pred_comp
 * (bts_components3d of the prediction).  lesion_vox (n int32, zeroed by the call, the layout of bts_component_sizes): lesion_vox[r] = the
 * truth voxels inside the dilated component of root r.  table (bts_lesion_pairs_table_bytes(capacity) = 16 capacity bytes, zeroed by the
 * call): `capacity` 64-bit keys (td_comp << 32) | pred_comp, 0 = empty, then `capacity` int32 pairs (reach, overlap) in the keys' slots:
 * for every distinct pair of a dilated component and a predicted component that share a voxel, the voxels they share and those of them
 * that are truth.  Integer atomics only: the counts are exact, the slot a pair lands in is not fixed.  status (two int64 on the device,
 * zeroed by the call): [0] = pairs stored, [1] = insertions that found no room.  A table that is too small is NO error: status[1] > 0,
 * status[0] + status[1] slots are enough for a rerun, every stored pair still holds its complete counts and lesion_vox is complete.
 * BTS_ERR_SHAPE for n outside [0, 2^31 - 1), K outside 2..8, a class_mask outside its range or a capacity outside 1..2^32. */
long bts_lesion_pairs_table_bytes(long capacity);
int bts_lesion_pairs(const int* td_comp, const uint8_t* truth, const int* pred_comp, long n, int K, int class_mask, int* lesion_vox,
                     void* table, long capacity, long* status, bts_stream_t stream);
/* boxes (nroots x 6 int32, every element written) = the half-open bounding box (d0,h0,w0,d1,h1,w1) of the component of comp (int32
 * (D,H,W) of bts_components3d) whose root is roots[i]; roots: nroots ASCENDING int32 on the device; (INT_MAX x 3, 0 x 3) for a root the
 * map does not hold.  BTS_ERR_SHAPE for a non-positive extent, D H W >= 2^31 - 1 or nroots outside 0..2^28; nroots == 0 launches nothing. */
int bts_component_boxes(const int* comp, int D, int H, int W, const int* roots, int nroots, int* boxes, bts_stream_t stream);
/* Two dense uint8 maps of the half-open box [d0,d1) x [h0,h1) x [w0,w1) of the volume (D,H,W), every byte written: g = 1 where the
 * voxel is of the truth region (K, class_mask) and of the dilated component of root td_root (td_comp == td_root + 1); m = 1 where
 * pred_comp's root is one of roots (nroots ASCENDING int32 on the device; nroots == 0: m is all 0 and roots may be NULL).  They feed
 * bts_region_surface(K = 2, class_mask = 2), bts_edt3d_sq and bts_masked_select.  BTS_ERR_SHAPE for a non-positive extent, D H W >=
 * 2^31 - 1, a box that is empty or leaves the volume, td_root outside the volume, K or class_mask as above, nroots outside 0..2^28. */
int bts_lesion_crop(const int* td_comp, const uint8_t* truth, const int* pred_comp, int D, int H, int W, int K, int class_mask, int d0,
                    int h0, int w0, int d1, int h1, int w1, int td_root, const int* roots, int nroots, uint8_t* g, uint8_t* m,
                    bts_stream_t stream);

/* ===== sliding-window inference with blended overlapping windows (the windowed form of test.py:128-148 and :164-178) =====
 * A launch carries B jobs, 1 <= B <= bts_window_batch_max(); a job is one augmented copy of one window: starts (3B HOST ints, (z0,y0,x0)
 * per job, each inside the volume; a window may hang over the volume's end), flips (B HOST ints, bits 4|2|1 = D|H|W as in bts_flip_affine).
 * The job table travels by value in the kernel arguments.  All tensors dense fp32, channels innermost.  BTS_ERR_SHAPE, before any HIP
 * call, for a non-positive extent, flip bits above 7, a start < 0 or >= its extent, a NULL table; BTS_ERR_UNSUPPORTED for B outside the cap. */
long bts_window_batch_max(void);
/* The input side of a windowed forward (test.py:164-178 pad, :107 normalise, :128-148 tf.reverse, for windows): from x (D,H,W,C),
 * out (B,R0,R1,R2,C): out[b, fd(d), fh(h), fw(w), c] = (v - mean[b,c]) / stdv[b,c] with v = x[z0+d, y0+h, x0+w, c] inside the volume and
 * v = 0 beyond its end (the raw intensities are padded BEFORE they are normalised, test.py:107,175: the overhang holds -mean/std).
 * mean, stdv: B*C HOST floats, a pair per job (channel TTA moves them per copy).  C <= 16 (BTS_ERR_UNSUPPORTED above).  Every element of
 * out is written; the window is read once per job. */
int bts_window_gather(const float* x, float* out, int D, int H, int W, int C, int R0, int R1, int R2, int B, const int* starts,
                      const int* flips, const float* mean, const float* stdv, bts_stream_t stream);
/* The output side (test.py:139-151 un-flip and average, with a window's importance): pred (B,R0,R1,R2,K) the network's output for the
 * jobs, still flipped; acc (D,H,W,K); nz (n0,R0), ny (n1,R1), nx (n2,R2) the normalised per-axis importance tables of
 * bts_amd.infer.window_plan on the device; rows (3B HOST ints): the table rows (iz,iy,ix) of each job's window.  For every voxel of a
 * job's window inside the volume: acc[z0+d, y0+h, x0+w, k] += ((scale * nz[iz][d]) * ny[iy][h]) * nx[ix][w] * pred[b, fd(d), fh(h), fw(w), k].
 * Owner computes: one thread owns an accumulator voxel, adds the jobs that hold it in list order and writes it once; no atomics, no race
 * between overlapping jobs, products and sums never contracted: one launch of B jobs gives the bits of B launches of one job.  Voxels
 * outside every window of the launch are not written.  BTS_ERR_UNSUPPORTED when acc and pred share memory; BTS_ERR_SHAPE also for a
 * table row outside its table. */
int bts_window_accumulate(const float* pred, float* acc, const float* nz, const float* ny, const float* nx, int n0, int n1, int n2, int D,
                          int H, int W, int K, int R0, int R1, int R2, int B, const int* starts, const int* flips, const int* rows,
                          float scale, bts_stream_t stream);
/* counts (n0*n1*n2 int32 on the device, zeroed by the call, window (iz,iy,ix) at (iz n1 + iy) n2 + ix) = the voxels with mask > 0 inside
 * each window of the plan, clipped to the volume: a window that counts 0 lies on voxels bts_tta_finish zeroes (test.py:154-155) and need
 * not be run.  mask (D,H,W) fp32; starts: n0+n1+n2 int32 ON THE DEVICE, the z, then y, then x starts.  Integer atomics: exact. */
int bts_window_occupancy(const float* mask, const int* starts, int* counts, int n0, int n1, int n2, int D, int H, int W, int R0, int R1,
                         int R2, bts_stream_t stream);

/* ===== training-time augmentation on the device (train.py:14-49) ===== */
/* per-channel mean / population variance of a (nvox, C) tensor with voxel stride ld (tf.nn.moments, train.py:18);
 * C <= 16; mean may be NULL; fp64 partials of x minus the first voxel's value (no cancellation against the mean: a constant volume
 * has variance exactly 0), fixed-order combine */
long bts_channel_moments_workspace(int C);
int bts_channel_moments(const float* x, float* mean, float* var, void* workspace, long workspace_bytes, long nvox, int C,
                        int ld, bts_stream_t stream);
/* xo = crop+flip of (x + shift[c]*sqrt(var[c])) * scale[c] (train.py:19-34), yo = one-hot of the cropped+flipped labels
 * without the background channel (train.py:38-41).  x: (S0,S1,S2,C), y: (S0,S1,S2) float labels, var: C device floats,
 * shift/scale: C HOST floats (the caller's random draws), window origin (o0,o1,o2), flip_mask bits 4|2|1 = axes 0|1|2. */
int bts_augment_crop(const float* x, const float* y, const float* var, float* xo, float* yo, int S0, int S1, int S2, int C,
                     int T0, int T1, int T2, int o0, int o1, int o2, int flip_mask, const float* shift, const float* scale,
                     int out_ch, bts_stream_t stream);
/* The same transformation for a whole batch in one launch, written straight into the batch tensors (no stack / permute copy
 * afterwards).  x, y, var: HOST arrays of N device pointers (volumes, labels, variances: one per example; all volumes (S0,S1,S2,C),
 * all crops (T0,T1,T2)); offsets: 3N host ints, flips: N host ints (bits 4|2|1), shift / scale: N*C host floats.
 * layout 0: xo (N,T0,T1,T2,C), yo (N,T0,T1,T2,out_ch); layout 1: xo (N,C,T0,T1,T2), yo (N,out_ch,T0,T1,T2).
 * The per-example table travels by value in the kernel arguments: bts_augment_batch_max() examples per launch, a larger N is split
 * into several launches by the call itself.  Per element the bits of bts_augment_crop (which is this call with N = 1, layout 0):
 * fmaf(shift, sqrtf(var), x) * scale.  BTS_ERR_SHAPE, before any HIP call, for N <= 0, C outside 1..16, out_ch <= 0, an empty crop,
 * a layout other than 0 / 1, a NULL table, flip bits above 7 or a window that leaves its volume. */
long bts_augment_batch_max(void);
int bts_augment_batch(const float* const* x, const float* const* y, const float* const* var, float* xo, float* yo, int N, int S0,
                      int S1, int S2, int C, int T0, int T1, int T2, const int* offsets, const int* flips, const float* shift,
                      const float* scale, int out_ch, int layout, bts_stream_t stream);
/* bts_augment_batch with a spatial transform per example: rotation + zoom + free-form deformation, as a gather in place of the copy,
 * in the same single launch.  For an output voxel t of a crop of extent T, from a source volume of extent S at window origin o:
 *   t~_k = flip_k ? T_k-1-t_k : t_k (the flip is undone first, as in bts_augment_batch), q = t~ - (T-1)/2,
 *   s = o + (T-1)/2 + M q + u(t~);  M = R0(th0) R1(th1) R2(th2) / z: rotations about axes 0, 1, 2 and the zoom z (z > 1 magnifies), built
 *   by the host in float64 and passed as 9 floats, row-major;
 *   u: a free-form deformation on a control grid of `spacing` voxels: g = t~/spacing, i = floor(g), f = g - i,
 *      u = sum_{a,b,c=0..3} B_a(f0) B_b(f1) B_c(f2) phi[i0+a, i1+b, i2+c, :], B the uniform cubic B-spline basis; phi has
 *      G_k = (T_k-1)/spacing + 4 (integer division) nodes per axis and 3 components, in source voxels, dense fp32 (G0,G1,G2,3) in DEVICE
 *      memory; NULL: no elastic part;
 *   image channels: trilinear at s, a corner outside the volume contributes fill[c] (scipy.ndimage mode='grid-constant'; a voxel
 *      whose eight corners are all outside is exactly fill[c]), then
 *      fmaf(shift, sqrtf(var), v) * scale on the interpolated value (var stays the variance of the whole untransformed volume);
 *   labels: the nearest voxel floor(s + 0.5), label 0 outside the volume; one-hot without the background as in bts_augment_batch.
 * An example whose spatial flag is 0 is copied inside the same launch, bit-equal to bts_augment_batch; one with M = I and phi = NULL
 * that takes the gather is bit-equal too (exact integer coordinates, weights exactly 0 and 1; finite volumes).  Coordinates are fp32; the
 * order of operations is written out above augment_spatial_batch_kernel (csrc/augment.hip) and bounds the error.
 * Arguments of bts_augment_batch plus per-example HOST arrays: spatial (N ints, 0 = copy), M (9N floats), phi (N device pointers or
 * NULLs), spacing (N ints), fill (N*C floats).  bts_augment_spatial_batch_max() examples per launch (the table entry is larger than
 * bts_augment_batch's); a larger N is split by the call itself.  No atomics: deterministic.  BTS_ERR_SHAPE, before any HIP call, for
 * everything bts_augment_batch rejects, a NULL table, a spacing < 1, a non-finite entry of M (every example is checked, whatever its
 * flag), or a phi with more than 256 nodes along axis 2. */
long bts_augment_spatial_batch_max(void);
int bts_augment_spatial_batch(const float* const* x, const float* const* y, const float* const* var, float* xo, float* yo, int N, int S0,
                              int S1, int S2, int C, int T0, int T1, int T2, const int* offsets, const int* flips, const float* shift,
                              const float* scale, const int* spatial, const float* M, const float* const* phi, const int* spacing,
                              const float* fill, int out_ch, int layout, bts_stream_t stream);

/* Class-location table of a label volume, for foreground-oversampled crops (no reference counterpart: train.py:26 crops uniformly; the
 * recipe is nnU-Net's).  y: V = S0*S1*S2 dense fp32 labels as the dataset stores them, label k in 1..out_ch = class k-1 (the convention
 * of bts_augment_crop's one-hot).  counts (out_ch int64): n_c = the voxels whose label is EXACTLY c+1 -- 0, a value above out_ch and a
 * non-integer value are in no class.  loc (out_ch x K int32): with s_c = max(1, ceil(n_c / K)) and m_c = ceil(n_c / s_c), entry j < m_c
 * is the linear index of the class's voxel of rank j s_c, ranks counting the class's voxels in ascending linear index; entries j >= m_c
 * are -1.  All out_ch*K entries and all counts are written on every call.  A pure function of the input, bit-identical from run to run:
 * a slot follows from the voxel's rank (count per workgroup, exclusive scan, second sweep), never from an atomic cursor; integer arithmetic
 * and plain stores only.  y is read twice.  BTS_ERR_SHAPE, before any HIP call: V < 1 or V >= 2^31, out_ch outside 1..8, K < 1, a NULL
 * y, counts or loc; BTS_ERR_WORKSPACE: a NULL workspace or one smaller than bts_class_locations_workspace() (itself BTS_ERR_SHAPE for a
 * V or out_ch the call refuses). */
long bts_class_locations_workspace(long V, int out_ch);
int bts_class_locations(const float* y, long* counts, int* loc, void* workspace, long workspace_bytes, long V, int out_ch, int K,
                        bts_stream_t stream);

/* Intensity augmentation of the batch that bts_augment_batch / bts_augment_spatial_batch wrote: Gaussian noise, Gaussian blur,
 * brightness, contrast and gamma (the nnU-Net / batchgenerators set; train.py:19-20 has only the shift and scale).  x: dense fp32
 * (N,T0,T1,T2,C) (layout 0) or (N,C,T0,T1,T2) (layout 1), 1 <= C <= 16, changed IN PLACE; labels are not touched.  The unit is one
 * (example n, channel c) volume v of T0*T1*T2 voxels, background included.  HOST tables: flags (N*C ints, a sum of BTS_INTENSITY_*),
 * params (N*C*5 floats: s, sigma, m, f, gamma), keys (2N uint32: the Philox key (k0,k1) of each example).  Stages in this order, each
 * on the output of the one before:
 *   NOISE     v[t] += s * z[e], s >= 0;  e = ((t0*T1 + t1)*T2 + t2)*C + c, the element's channels-last index in EITHER layout (so both
 *             layouts get the same noise);  z: Philox4x32-10 of key (k0,k1) and counter (q & 0xffffffff, q >> 32, 0, 0), q = e >> 2,
 *             element e takes output word e & 3; words (0,1) and (2,3) are Box-Muller pairs: u1 = ((w_a >> 8) + 1) 2^-24,
 *             u2 = (w_b >> 8) 2^-24, r = sqrt(-2 ln u1), z_a = r cos(2 pi u2), z_b = r sin(2 pi u2)  (logf / sinf / cosf, not the fast
 *             intrinsics; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85);
 *   BLUR      scipy.ndimage.gaussian_filter(v, sigma) with its defaults: separable, radius r = int(4 sigma + 0.5), weights
 *             exp(-j^2 / (2 sigma^2)) normalised in float64 on the host (bts_intensity_blur_weights) and passed as floats,
 *             mode='reflect' (d c b a | a b c d | d c b a, period 2n when r >= n); r <= 16; out of place through the workspace;
 *   BRIGHT    v *= m, m > 0  (alone: bit-equal to the fp32 product);
 *   CONTRAST  batchgenerators augment_contrast, preserve_range: mu = mean(v), lo = min(v), hi = max(v),
 *             v = clip((v - mu) f + mu, lo, hi);
 *   GAMMA     batchgenerators augment_gamma, retain_stats, epsilon 1e-7: with INVERT v = -v;  mu, sd = mean, population std of v,
 *             lo = min(v), R = max(v) - lo;  v = ((v - lo) / (R + 1e-7))^gamma R + lo;  v = (v - mean(v)) / (std(v) + 1e-8) sd + mu;
 *             with INVERT v = -v.  A constant volume comes out unchanged up to the rounding of the last line.
 * Means and deviations are fp64 sums of v - v[0] and its square in a fixed order (a constant volume has deviation exactly 0), min and
 * max are exact; no floating-point atomics.  The result of an example depends neither on N, nor on its place in the batch, nor on the
 * layout, nor on how many launches the call makes (the job table travels by value, 32 (n,c) volumes per launch; any N works); two
 * runs are bit-identical.  An (n,c) without a flag is not written.  The fp32 order of operations is written out at the head of
 * csrc/intensity.hip and bounds the error.
 * BTS_ERR_SHAPE, before any HIP call: N <= 0, C outside 1..16, an empty crop (or one of about 2^31 / C voxels or more), a layout other than 0 / 1, a NULL x, table or key array,
 * a workspace smaller than bts_intensity_batch_workspace(), an unknown flag bit, and on an enabled stage a non-finite or negative s,
 * sigma <= 0 or r > 16, a non-finite or non-positive m, f or gamma. */
#define BTS_INTENSITY_NOISE 1
#define BTS_INTENSITY_BLUR 2
#define BTS_INTENSITY_BRIGHT 4
#define BTS_INTENSITY_CONTRAST 8
#define BTS_INTENSITY_GAMMA 16
#define BTS_INTENSITY_INVERT 32
long bts_intensity_batch_workspace(int N, int T0, int T1, int T2, int C);
/* host only: the blur radius of sigma (-1: sigma <= 0, not finite, or r > 16) and, unless NULL, its r + 1 weights w[|j|] */
long bts_intensity_blur_weights(float sigma, float* weights);
int bts_intensity_batch(float* x, int N, int T0, int T1, int T2, int C, int layout, const int* flags, const float* params,
                        const uint32_t* keys, void* workspace, long workspace_bytes, bts_stream_t stream);

/* ===== the nested BraTS regions as targets and as the decoded prediction (no reference counterpart: train.py:38-41 trains its
 * per-channel sigmoids on disjoint one-hot labels, test.py:259-261 decodes an arg-max) =====
 * Channels are (WT, TC, ET) = labels {1,2,4}, {1,4}, {4}, the order of bts_amd.infer.BRATS_REGIONS.  All three calls are single streaming
 * passes defined for C == 3 only: another C returns BTS_ERR_UNSUPPORTED, a non-positive extent or a voxel stride below C BTS_ERR_SHAPE,
 * both before any HIP call.  A channels-last voxel is 12 bytes: a lane takes four voxels as three 16-byte accesses where the base
 * pointers are 16-byte aligned, the last (voxels mod 4) voxels and unaligned views (a batch inside a larger buffer) go voxel by voxel;
 * the results do not depend on the path. */
/* y, the dense label batch bts_augment_crop / bts_augment_batch / bts_augment_spatial_batch wrote (one-hot minus the background), IN
 * PLACE: (l1, l2, l3) -> ((l1 + l2) + l3, l1 + l3, l3).  channels_first 0: (N, V, 3); 1: (N, 3, V), V the voxels of one example; 16-byte
 * accesses along the planes of every example whose three plane starts are aligned.  A NULL y is BTS_ERR_SHAPE. */
int bts_region_targets(float* y, int N, long V, int C, int channels_first, bts_stream_t stream);
/* the hard Dice counts of the regions: per region r, P_r = #(p_r > 0.5), T_r = #(t_r > 0.5), I_r = # of voxels where both hold;
 * table[3r + 0..2] = (I_r, P_r, T_r) as doubles (zeroed by the call): what bts_dice_metric_value(table, out, W, 3, 0) reduces, one cell
 * per region, to macro = mean_r (2 I_r + 1) / (P_r + T_r + 1) and micro = sum I / (sum P + sum T) (util.py:54-55).  y_true, y_pred: NV
 * voxels, channel stride 1, voxel strides ldt, ldp.  Counted in integer registers, summed over wave and workgroup, one add per
 * workgroup and entry: integers below 2^53, so the table is exact and bit-identical from run to run.  labels (NV uint8, or NULL): the
 * decode of bts_region_finish with p > 0.5 in the coding of bts_dice_metric_sums' map: 0, 1, 2, and 3 (not 4) for ET. */
int bts_region_dice_sums(const float* y_true, const float* y_pred, uint8_t* labels, double* table, long NV, int C, int ldt, int ldp,
                         bts_stream_t stream);
/* the counterpart of bts_tta_finish for a network trained on regions: y = prob * bmask and/or the label map by the overwrite rule of
 * the BraTS conversions, on the masked probabilities: 4 if et >= threshold, else 1 if tc >= threshold, else 2 if wt >= threshold, else
 * 0, and 0 wherever bmask == 0.  Deliberately NOT the nested rule (ET only inside TC inside WT).  decode(encode(L)) = L for every map L
 * over {0,1,2,4}.  prob, y: dense (nvox, 3); bmask: one float per voxel; y and labels may each be NULL. */
int bts_region_finish(const float* prob, const float* bmask, float* y, uint8_t* labels, long nvox, int C, float threshold,
                      bts_stream_t stream);

/* ===== ensembles of tumour models and voxel-wise uncertainty maps (bts_amd.infer.StageEnsemble, uncertainty_scores; DESIGN section 37.
 * The reference runs one checkpoint, test.py:185-221, and reports a label per voxel) =====
 * Welford's recurrence over the n floats of member k's mean probabilities (k counts from 1): d = p - mean; mean += d / k;
 * m2 += d * (p - mean), every operation rounded once, so the float32 numpy recurrence bit for bit.  k == 1 writes mean = p and m2 = 0 and
 * does not read the accumulators.  m2 may be NULL: only the mean is kept.  After M members mean is their mean and m2 the sum of their
 * squared deviations from it.  BTS_ERR_SHAPE for n <= 0, k < 1 or a missing p or mean; BTS_ERR_UNSUPPORTED when two of the buffers are
 * the same. */
int bts_ensemble_update(const float* p, float* mean, float* m2, long n, int k, bts_stream_t stream);
/* unc (nvox, C) uint8, channels last = one level 0..100 per voxel and channel, 0 where bmask (one float per voxel) == 0.
 * mode 0, entropy: p = clamp(mean, 0, 1), h = -(p log2 p + (1 - p) log2(1 - p)), 0 at p in {0, 1}; level = min(100, floor(100 h + 0.5));
 * spread is not read.  mode 1, deviation: level = min(100, floor(200 sqrt(max(spread, 0) * scale) + 0.5)), spread = bts_ensemble_update's
 * m2 with scale = 1 / M, or a variance with scale = 1; the population deviation of values in [0, 1] is at most 0.5; mean is not read.
 * BTS_ERR_UNSUPPORTED for another mode; BTS_ERR_SHAPE for nvox <= 0, C outside 1..1024, a negative scale or a missing buffer. */
int bts_uncertainty_finish(const float* mean, const float* spread, const float* bmask, uint8_t* unc, long nvox, int C, int mode,
                           float scale, bts_stream_t stream);
/* table (C, 101, 4) uint64 on the device, accumulated across calls: per voxel with mask != 0 (mask may be NULL: every voxel) and per
 * channel c, table[c][min(unc[v C + c], 100)][2 t + pr] += 1 with t = bit min(truth[v], K-1) of class_masks[c] and pr the same of
 * pred[v] (cells TN, FP, FN, TP).  truth, pred, mask: dense uint8 label maps; class_masks: C HOST values below 2^K; C in 1..4, K in 2..8.
 * Integer atomics only: exact and bit-reproducible.  BTS_ERR_UNSUPPORTED for C outside 1..4; BTS_ERR_SHAPE for K outside 2..8, nvox
 * outside [0, 2^31 - 1) or a class mask outside its range; nvox == 0 launches nothing. */
int bts_uncertainty_confusion(const uint8_t* truth, const uint8_t* pred, const uint8_t* unc, const uint8_t* mask, long nvox, int C, int K,
                              const unsigned* class_masks, unsigned long long* table, bts_stream_t stream);

/* ===== dataset preprocessing on the device (preprocess.py:17-131: create_dataset, compute_norm, main) =====
 * Dense fp32 (S0,S1,S2,C) volumes, C innermost, 1 <= C <= 16.  A crop window (T0,T1,T2,C) of such a volume is addressed in place:
 * `xwin` points at its origin, st0 / st1 are the element strides of the two outer axes, the voxel stride is C. */
/* bounding-box search of preprocess.py:39-49 (np.any per plane): occ (S0+S1+S2 ints, axis 0 first) gets a 1 for every plane index
 * of every axis that holds an x != 0 (NaN counts, -0.0 does not).  Flags are only ever set: zero occ once and run every case into
 * it for the box of a whole dataset. */
int bts_prepro_occupancy(const float* x, int* occ, int S0, int S1, int S2, int C, bts_stream_t stream);
/* the accumulations of compute_norm (preprocess.py:75-77, 81-82) over one window, in fp64, fixed order, no float atomics.
 * mean_or_null == NULL: acc[0:C] += sum x, acc[C:2C] += #(x > 0) (an exact double).
 * mean_or_null = C device doubles: acc[0:C] += sum (double(x) - mean[c])^2.  acc: device doubles, accumulated in call order. */
long bts_prepro_workspace(int C);
int bts_prepro_sums(const float* xwin, long st0, long st1, int T0, int T1, int T2, int C, const double* mean_or_null, double* acc,
                    void* workspace, long workspace_bytes, bts_stream_t stream);
/* the stored example of preprocess.py:122-130: xo (T0,T1,T2,C) = float((double(x) - mean[c]) / std[c]) (IEEE fp64 subtract and
 * divide, one rounding to fp32), yo (T0,T1,T2) = y >= 4 ? 3 : y (preprocess.py:36).  ywin: the same window of the (S0,S1,S2) label
 * volume with element strides yst0 / yst1, voxel stride 1; ywin and yo may both be NULL.  mean, stdv: C device doubles. */
int bts_prepro_crop_norm(const float* xwin, const float* ywin, long st0, long st1, long yst0, long yst1, int T0, int T1, int T2,
                         int C, const double* mean, const double* stdv, float* xo, float* yo, bts_stream_t stream);

/* ===== per-case normalisation over the voxels inside a mask, with optional percentile clipping (bts_amd.ops.case_norm) =====
 * xwin: a window (T0,T1,T2,C) addressed as above.  mask_or_null: the same window of a fp32 (S0,S1,S2) volume with element strides
 * mst0 / mst1, non-zero = inside; NULL: a voxel is inside when any of its channels is > 0 (test.py:53-54).  n = voxels inside.  Per
 * channel c, with s the inside values in ascending order: with clip != 0, lo_c / hi_c = s[k] + f (s[min(k+1,n-1)] - s[k]) for
 * h = (n-1) p / 100, k = floor(h), f = h - k and p = p_lo / p_hi, in fp64; with clip == 0, -inf / +inf.  v = clamp(double(x), lo_c, hi_c),
 * mean_c = sum v / n, std_c = sqrt(sum (v - mean_c)^2 / n) (two passes, fp64, fixed order: the same bits in every run).
 * xo (T0,T1,T2,C), dense, every element written = float((v - mean_c) / std_c) inside (one rounding), +0.0 outside, +0.0 throughout a
 * channel with std_c == 0 and everywhere when n == 0.  yo (T0,T1,T2) = y >= 4 ? 3 : y of the label window ywin_or_null (strides yst0 /
 * yst1); both may be NULL.  stats: 1 + 4 C device doubles, n then (mean, std, lo, hi) per channel; all 0 when n == 0.
 * The order statistics are exact: a four-pass radix select on the order-preserving 32-bit key of the float, all channels and both
 * bounds in the same passes, integer histograms.  Nothing leaves the stream; no host round trip.  Inputs are expected to be finite.
 * workspace: device memory of exactly bts_case_norm_workspace(C) bytes (negative for C outside 1..16); nothing in it need be set.
 * bts_case_norm_blocks(): the grid cap of the voxel-owning kernels (256 voxels per workgroup and sweep, one fp64 partial each).
 * BTS_ERR_SHAPE, before any HIP call: C outside 1..16, a non-positive extent, a stride smaller than the rows it spans, more than
 * 2^31 - 1 voxels, a row of 2^28 floats or more, clip with a percentile outside [0,100] or p_lo > p_hi, a NULL xwin, xo or stats, ywin
 * without yo.  BTS_ERR_WORKSPACE: a NULL or short workspace. */
long bts_case_norm_workspace(int C);
int bts_case_norm_blocks(void);
int bts_case_norm(const float* xwin, long st0, long st1, const float* mask_or_null, long mst0, long mst1, const float* ywin_or_null,
                  long yst0, long yst1, int T0, int T1, int T2, int C, int clip, double p_lo, double p_hi, float* xo, float* yo,
                  double* stats, void* workspace, long workspace_bytes, bts_stream_t stream);

/* ===== rigid co-registration of a scan's modalities by mutual information (bts_amd.coreg; the reference stacks its modalities voxel
 * for voxel, test.py:21-42, and so relies on files that were registered beforehand) =====
 * q (n bytes, dense) = clamp(floor((double(x) - lo) * bins / (hi - lo)), 0, bins - 1) of the n dense fp32 values x, evaluated in fp64, each
 * operation rounded once; a NaN gives bin 0.  lo < hi: host doubles; bins in 2..64.
 * BTS_ERR_SHAPE, before any HIP call: n <= 0, hi <= lo or a bound that is not finite, bins outside 2..64, a NULL pointer. */
int bts_quantize_bins(const float* x, uint8_t* q, long n, double lo, double hi, int bins, bts_stream_t stream);
/* K joint histograms of the binned volumes qf (Df,Hf,Wf) and qm (Dm,Hm,Wm), dense bytes below `bins`, one per candidate map, by
 * partial-volume interpolation (Collignon / Maes): hist, K x bins x bins device 64-bit counts, [k][fixed bin][moving bin], is overwritten
 * completely and need not be set.  m12: a HOST array of 12 K doubles read during the call, K row-major 3 x 4 maps from a fixed voxel
 * coordinate to a moving voxel coordinate (m12 of bts_affine_resample3d).  The lattice: points f = o + l * s of the fixed grid, 0 <= l_j < n_j,
 * with o_j >= 0, s_j >= 1, n_j >= 1 and o_j + (n_j - 1) s_j <= extent_j - 1.  With Q = 32, per point and candidate, a = qf[f]:
 *   c_j = ((m[j][0] f0 + m[j][1] f1) + m[j][2] f2) + m[j][3] in fp64, every operation rounded once (no fused multiply-add);
 *   the point counts only if 0 <= c_j <= N_j - 1 on all three axes; then i_j = floor(c_j), r_j = (int)floor((c_j - i_j) Q + 0.5) in [0, Q];
 *   the corner (d0,d1,d2) in {0,1}^3 holds b = qm[min(i_j + d_j, N_j - 1)], and hist[k][a][b] grows by prod_j (d_j ? r_j : Q - r_j).
 * Every counted point adds exactly Q^3 = 32768, so the overlap of candidate k is sum(hist[k]) / 32768 points.  All sums are integers: the
 * result is the same bits in every run.  No workspace.  A byte of qf / qm at or above `bins` counts as bins - 1.
 * BTS_ERR_SHAPE, with nothing launched: a non-positive extent or a volume of 2^31 voxels or more, a lattice that is not as above, K outside
 * 1..32, bins outside 2..64, a NULL qf, qm, m12 or hist. */
int bts_joint_hist_pv(const uint8_t* qf, int Df, int Hf, int Wf, const uint8_t* qm, int Dm, int Hm, int Wm, int o0, int o1, int o2, int s0,
                      int s1, int s2, int n0, int n1, int n2, const double* m12, int K, int bins, unsigned long long* hist,
                      bts_stream_t stream);

/* ===== N4 bias-field correction of one MRI volume (bts_amd.n4; Tustison et al. 2010.  The reference has no such stage:
 * preprocess.py and test.py take the scans as they come) =====
 * The volume x is dense fp32 (D,H,W).  The bias field is exp of a cubic B-spline with M_a mesh elements and M_a + 3 control points per axis,
 * phi: (M0+3)(M1+3)(M2+3) device doubles, last axis fastest.  Along an axis of extent N a voxel of index p has u = (p + 0.5) / N * M,
 * cell i = min(floor(u), M - 1), t = u - i, and the uniform cubic B-spline weights of t, (1-t)^3/6, (3t^3-6t^2+4)/6, (-3t^3+3t^2+3t+1)/6,
 * t^3/6, multiply the control points i .. i+3.  The working lattice is the strided sub-grid p = s_a / 2 + l s_a, 0 <= l < n_a =
 * (N_a - 1 - s_a / 2) / s_a + 1, with 1 <= s_a <= N_a; a lattice array is n0 n1 n2 values, last axis fastest.  All arithmetic is fp64, every
 * operation rounded once (no fused multiply-add), no floating-point atomics, fixed summation orders: the same bits in every run.
 * Every entry point returns BTS_ERR_SHAPE with nothing launched for a non-positive extent, a volume of 2^31 voxels or more, a stride
 * outside 1..extent, a mesh outside 1..64, bins outside 2..1024, npts outside 1..2^31-1, or a NULL pointer that is not marked _or_null. */
/* v = log(double(x)) and lmask = 1 at the lattice points where x > 0 and finite and mask_or_null (D,H,W bytes, non-zero = inside; NULL: all)
 * allows it; v = 0, lmask = 0 elsewhere. */
int bts_n4_log_lattice(const float* x, const uint8_t* mask_or_null, int D, int H, int W, int s0, int s1, int s2, double* v, uint8_t* lmask,
                       bts_stream_t stream);
/* r = v - f on the mask (0 elsewhere); range4[0], range4[1] = the exact min lo and max hi of r over the mask (+inf, -inf for an empty mask),
 * range4[2..3] are the call's own scratch; hist: `bins` 64-bit counts, overwritten.  With sl = (hi - lo) / (bins - 1), a masked point has
 * c = (r - lo) / sl, i = min(floor(c), bins - 2), o = c - i, q = rint(o 2^24), and adds 2^24 - q to bin i and q to bin i + 1; with hi == lo
 * every point adds 2^24 to bin 0.  Three launches. */
int bts_n4_range_hist(const double* v, const double* f, const uint8_t* lmask, long npts, int bins, double* r, double* range4,
                      long long* hist, bts_stream_t stream);
/* res = r - (E[i] (1 - o) + E[i+1] o) on the mask with i, o as above from the host doubles lo and sl >= 0 (0 elsewhere); E: `bins` device
 * doubles, the sharpened table. */
int bts_n4_residual(const double* r, const uint8_t* lmask, const double* E, long npts, int bins, double lo, double sl, double* res,
                    bts_stream_t stream);
/* one level of multilevel B-spline approximation (Lee, Wolberg, Shin 1997) in gather form.  A masked lattice point with residual z and
 * tensor weight w_c at control point c has S = the product over the axes of the sum of its four squared weights; num[c] = sum w_c^3 z / S,
 * den[c] = sum w_c^2 over the lattice points whose cell lies in the 4-cell support of c, dphi[c] = num / den, 0 where den == 0;
 * phi_or_null[c] += dphi[c].  One workgroup per control point; at most 512 lattice points per axis. */
int bts_n4_fit(const double* res, const uint8_t* lmask, int D, int H, int W, int s0, int s1, int s2, int M0, int M1, int M2, double* num,
               double* den, double* dphi, double* phi_or_null, bts_stream_t stream);
/* f_new = the spline at every lattice point; parts: bts_n4_eval_parts(npts) pairs of doubles, the sums of e = exp(f_new - f_old) and of
 * e^2 over the masked points of each run of 1024 lattice points, to be added up in order by the caller. */
long bts_n4_eval_parts(long npts);
int bts_n4_eval(const double* phi, int D, int H, int W, int s0, int s1, int s2, int M0, int M1, int M2, const double* f_old,
                const uint8_t* lmask, double* f_new, double* parts, bts_stream_t stream);
/* out = float(double(x) / exp(spline)) at every voxel; field_or_null = float(exp(spline)).  x is read once and out written once. */
int bts_n4_apply(const float* x, int D, int H, int W, const double* phi, int M0, int M1, int M2, float* out, float* field_or_null,
                 bts_stream_t stream);

/* library identification */
const char* bts_version(void);

/* ===== optional in-library timing of the two dominant kernels (bench.py roofline) ===== */
/* HIP events recorded on the launch stream immediately around igemm_kernel / wgrad_kernel launches.
 * bts_profile_enable(1) clears and starts recording, (0) stops; read the records after synchronising the stream.
 * sym: 0..4 = igemm_kernel<2,1,4,1|2,2,4,1|1,2,2,2|1,1,2,2|1,1,4,1>, +8 = its 1x1x1 staging variant; 100/101 = wgrad_kernel<true/false> */
int bts_profile_enable(int on);
int bts_profile_count(void);
int bts_profile_get(int i, int* sym, double* flops, float* ms);

/* ===== reduced-precision STORAGE path of the forward pass (BASELINE configs[4]: fp16 full-volume inference, VAE off: model.py:67-68,
 * test.py:128-134; forward half of configs[2], bf16).  Activations and packed weights are 16-bit, every sum is fp32
 * (v_mfma_f32_32x32x16_{f16,bf16}; GroupNorm statistics, gates and the sigmoid head in fp32 from the stored values).  The reference has
 * no such mode: the parity reference of these entry points is the fp32 engine above.  `ld` arguments count ELEMENTS. ===== */
#define BTS_LP_F16 1
#define BTS_LP_BF16 2
/* packed weight image of a conv kind: [tap][16-cin step][32-cout block][k half][32 couts][8 cin]; same folding arguments as bts_conv_pack */
long bts_lp_packed_bytes(int kind, int role, int Cin_slab, int Cout);
int bts_lp_pack(int kind, int role, int dtype, const float* w, void* wp, int Cin_ref, int Cout, int Cin_slab, int dup_start,
                int dup_shift, bts_stream_t stream);
/* y = conv(x) + bias (resnet.py:30-37,80-87,96-103; downsample.py:28-35; upsample.py:28-33).  Cin % 16 == 0; views' strides % 8 == 0 */
/* workspace (may be NULL / 0): lets stride-1 grids too small to fill the chip split the input channels over workgroups (fp32 partial
 * sums, fixed-order reduce); size from bts_lp_conv3d_workspace (0 when the shape does not need it) */
long bts_lp_conv3d_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout);
int bts_lp_conv3d_fwd(int kind, int dtype, const void* x, const void* wp, const float* bias, void* y, void* workspace, long workspace_bytes,
                      int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldy, bts_stream_t stream);
/* dx (+)= conv^T(dy) in the storage type (the data gradients TF autodiff derives, train.py:142-151); (D,H,W) are the forward INPUT
 * dims, wp_bwd = bts_lp_pack(kind, BTS_ROLE_BWD_DATA, ...); Cout % 16 == 0 */
long bts_lp_conv3d_bwd_data_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout);
int bts_lp_conv3d_bwd_data(int kind, int dtype, const void* dy, const void* wp_bwd, void* dx, void* workspace, long workspace_bytes,
                           int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy, int accum, bts_stream_t stream);
/* dx (+)= conv3x3x3^T(dy) + conv1x1x1^T(dy2) in ONE launch: the data gradients of the two convolutions that read a ResnetBlock's input
 * (conv1 resnet.py:80-87 and the shortcut resnet.py:96-103, both applied to `inputs`: resnet.py:118,134) meet in dx under train.py:151.
 * The shortcut's contraction rides on conv1's as an extra K-segment at the centre tap (1/27 more matrix work) with dy2 read straight
 * into the matrix instruction -- instead of a second launch that read-modify-writes the Cin-wide dx.  dy / dy2: (N,D,H,W,Cout), voxel
 * strides lddy / lddy2; wp_bwd / wp2_bwd = bts_lp_pack(K3S1 / K1, BTS_ROLE_BWD_DATA, ...) with the same Cin_slab and fold.  Shapes the
 * fused kernels do not take run as the two launches (the call always completes); *fused (may be NULL) = 1 if the one-launch form ran.
 * dx_split (elements; 0 = dx is one (N,D,H,W,Cin) view): columns [32 b, 32 b + 32) go to dx + b * dx_split, every block a tensor of its
 * own with voxel stride lddx -- the gradient of the decoder's concat of 32-channel tensors (decoder.py:75) leaves as DENSE tensors whose
 * readers fetch whole 128-byte lines.  Only the fused tiled kernel writes that form: bts_lp_conv3d_bwd_data_sc_split_ok (1 / 0) says
 * whether it takes the shape; BTS_ERR_UNSUPPORTED otherwise.  BTS_LP_SC=0 in the environment: always the two launches (A/B aid) */
long bts_lp_conv3d_bwd_data_sc_workspace(int N, int D, int H, int W, int Cin, int Cout);
int bts_lp_conv3d_bwd_data_sc_split_ok(int N, int D, int H, int W, int Cin, int Cout);
int bts_lp_conv3d_bwd_data_sc(int dtype, const void* dy, const void* wp_bwd, const void* dy2, const void* wp2_bwd, void* dx, long dx_split,
                              void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int lddx, int Cout, int lddy,
                              int lddy2, int accum, int* fused, bts_stream_t stream);
/* The weight gradients of the TWO convolutions that read a ResnetBlock's input (resnet.py:134 conv1, 3x3x3; resnet.py:118 shortcut, 1x1x1)
 * from ONE pass over that input (train.py:151): dw3 (+)= from dy3 as bts_lp_conv3d_bwd_weight(K3S1), dw1 (Keras layout (1,1,1,Cin_ref,Cout))
 * (+)= sum_v x[v][c] dy1[v][k] -- one more accumulator per wave of the streaming kernel, fed by the centre-tap fragments of x it reads anyway;
 * the HBM-bound 1x1x1 weight-gradient launch and its own read of the Cin-wide x go away.  db3 (may be NULL; dy3 dense then) (+)= sum dy3.
 * dup_start / dup_shift fold both kernels alike.  x_split (elements; 0 = one tensor): x as a list of Cin / 32 dense 32-channel tensors x +
 * b * x_split with voxel stride ldx (the operands of a concat; no fold then).  Workspace query -1 / return value 1 (nothing launched) outside the streaming kernel's
 * shapes (W % 32, H % 8, large volumes): run bts_lp_conv3d_bwd_weight twice. */
long bts_lp_conv3d_bwd_weight_pair_workspace(int N, int D, int H, int W, int Cin, int Cout);
int bts_lp_conv3d_bwd_weight_pair(int dtype, const void* x, long x_split, const void* dy3, const void* dy1, float* dw3, float* dw1, float* db3,
                                  void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy3,
                                  int lddy1, int dup_start, int dup_shift, int accumulate, bts_stream_t stream);
/* dw (fp32, Keras layout (kd,kh,kw,Cin_ref,Cout)) (+)= the weight gradient of a stride-1 3x3x3 / 1x1x1 conv from 16-bit x and dy
 * (voxel contraction on the 16-bit matrix pipe, fp32 partials, fixed-order finalize); db (may be NULL; dy dense then) (+)= sum dy.
 * dup_start / dup_shift as bts_conv_pack: Cin + dup_shift == Cin_ref, both copies of the folded slice receive the gradient.
 * The strided kinds too (no fold): x on the forward-input grid (D,H,W), dy on the half grid (K3S2, even sizes) or the doubled grid (K3S2T),
 * dw in the layer's own Keras layout.  BTS_ERR_SHAPE for channel counts or strides that are not multiples of 8: run
 * bts_conv3d_bwd_weight on widened copies.
 * This call, bts_lp_conv3d_bwd_weight_pair and bts_lp_conv3d_gnin_bwd_weight choose their kernel and validate EVERYTHING before the first
 * launch: a call that returns an argument status (also for a db that cannot be produced -- BTS_ERR_UNSUPPORTED where lddy != Cout,
 * BTS_ERR_SHAPE where Cout > 256 or Cout / 8 does not divide 256) has not touched dw, whatever `accumulate` says. */
long bts_lp_conv3d_bwd_weight_workspace(int kind, int N, int D, int H, int W, int Cin, int Cout);
/* Host-only query, asked before anything runs (a trainer decides the fp32 route from it): 1 when the argument rules above pass for the dense,
 * aligned, unfolded call on a (D,H,W) forward input -- channel counts in whole 16-byte chunks, even extents for BTS_CONV_K3S2, and for
 * BTS_CONV_K3S1 / BTS_CONV_K1, whose callers ask for db, a Cout <= 256 with Cout / 8 dividing 256 -- else 0, also for an unknown kind.
 * Not a status.  (The strided kinds are asked without the db rule: their callers always were.) */
int bts_lp_conv3d_bwd_weight_args_ok(int kind, int D, int H, int W, int Cin, int Cout);
int bts_lp_conv3d_bwd_weight(int kind, int dtype, const void* x, const void* dy, float* dw, float* db, void* workspace, long workspace_bytes,
                             int N, int D, int H, int W, int Cin, int ldx, int Cout, int lddy, int dup_start, int dup_shift, int accumulate,
                             bts_stream_t stream);
/* fp32 <-> storage type, `rows` rows of C elements with row strides (the 2-channel input block runs in fp32: K = 16 is its floor) */
int bts_lp_cast(int dtype, const float* src, long ld_src, void* dst, long ld_dst, long rows, int C, bts_stream_t stream);
/* encoder.py:39,71 (Dropout(rate) on the input volume) AND the cast of the dense (rows, C <= 4) fp32 volume into the zero-padded 16-channel
 * matrix step, in one pass: element i is kept (scaled by 1 / (1 - rate)) where bts_dropout_mask's generator says so for the same (seed, i)
 * -- bit-identical to bts_dropout_mask + bts_dropout_apply + bts_lp_cast_pad16, without the mask and the dropped volume being written */
int bts_lp_dropout_cast_pad16(int dtype, const float* src, void* dst, long rows, int C, float rate, uint64_t seed, bts_stream_t stream);
int bts_lp_uncast(int dtype, const void* src, long ld_src, float* dst, long ld_dst, long rows, int C, bts_stream_t stream);
/* fp32 rows of C <= 4 channels -> dense storage-type rows of 16 channels with a zero tail, in one pass: the 2-channel input volume
 * (model.py:58, after encoder.py:71's dropout), the 2-channel VAE-output gradient and the 1-channel VAE tensor (vae.py:110-111) as
 * whole 16-channel matrix steps */
int bts_lp_cast_pad16(int dtype, const float* src, long ld_src, void* dst, long rows, int C, bts_stream_t stream);
/* GroupNormalization (group_norm.py:83-124), both semantics; x dense; G > 0 and G | C (BTS_ERR_SHAPE otherwise, also in the epilogues and
 * backward passes below that take G) */
long bts_lp_gn_workspace(int N, long V, int C, int G);
int bts_lp_gn_stats(int dtype, const void* x, float* mean, float* rstd, void* workspace, long workspace_bytes, int N, long V, int C, int G,
                    int mode, float eps, bts_stream_t stream);
int bts_lp_gn_apply(int dtype, const void* x, void* y, const float* gamma, const float* beta, const float* mean, const float* rstd, int N,
                    long V, int C, int ldy, int G, int mode, int relu, bts_stream_t stream);
/* GroupNormalization backward (slab semantics; fused ReLU mask when relu != 0): dx in the storage type and, when dx32 != NULL, the same
 * values in fp32 (for a weight gradient that still runs on the fp32 matrix pipe); dgamma / dbeta fp32 (+= when accumulate_params).
 * dbias (may be NULL, C floats, += when accumulate_params): column sums of dx over voxels and samples = the bias gradient of the conv
 * whose output this layer normalised (resnet.py:80-93: conv -> GroupNormalization), taken from the same pass.
 * BTS_ERR_UNSUPPORTED for shapes outside its tiling (group length not a multiple of 2048, C/G > 32): run bts_gn_bwd on widened copies */
long bts_lp_gn_bwd_workspace(int N, long V, int C, int G);
/* Host-only query: 1 when V voxels of C channels in G slab-mode groups fit that tiling (whole 2048-element steps per (sample, group), a
 * power-of-two C <= 256, C / G <= 32 dividing 256), else 0; not a status.  The same rule holds for bts_lp_conv3d_bwd_data_gn_bwd and
 * bts_lp_block_bwd: a caller asks it before choosing between them and the fp32 kernels. */
int bts_lp_gn_bwd_tiled(long V, int C, int G);
int bts_lp_gn_bwd(int dtype, const void* x, const void* dy, void* dx, float* dx32, const float* gamma, const float* beta, const float* mean,
                  const float* rstd, float* dgamma, float* dbeta, void* workspace, long workspace_bytes, int N, long V, int C, int lddy, int G,
                  int relu, int accumulate_params, float* dbias, bts_stream_t stream);
/* A ResnetBlock's conv2 data gradient and its GroupNorm-1 (+ReLU) backward as one entry point (resnet.py:80-93 in reverse under
 * train.py:151; replaces bts_lp_conv3d_bwd_data followed by bts_lp_gn_bwd): da = conv3x3x3^T(dy) is stored dense (N,D,H,W,Cg) in the
 * storage type, dc / dc32 / dgamma / dbeta / dbias are bts_lp_gn_bwd's outputs for x = c, dy = da.  Where the z-marching kernel takes
 * the layer the class sums GroupNorm's backward starts from leave the conv's epilogue (one read of c per stored row) instead of a
 * reduce pass over da and c; elsewhere the two run back to back -- same results up to the order of the fp32 class sums.
 * Cg = GroupNorm channels = the forward conv's input channels, Cdy = dy's channels (rows of lddy); wp_bwd = bts_lp_pack(BTS_CONV_K3S1,
 * BTS_ROLE_BWD_DATA, ...); *fused_out (may be NULL) <- 1 | 0: which form ran.  Error codes as bts_lp_gn_bwd. */
long bts_lp_conv3d_bwd_data_gn_bwd_workspace(int N, int D, int H, int W, int Cg, int Cdy, int G);
int bts_lp_conv3d_bwd_data_gn_bwd(int dtype, const void* dy, const void* wp_bwd, void* da, const void* c, void* dc, float* dc32,
                                  const float* gamma, const float* beta, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                                  void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cg, int Cdy, int lddy, int G, int relu,
                                  int accumulate_params, float* dbias, int* fused_out, bts_stream_t stream);
/* GlobalAveragePooling3D of the shortcut (resnet.py:45-46,121): out[n][c] = scale * sum_v x */
long bts_lp_colsum_workspace(int N, long V, int C);
int bts_lp_colsum(int dtype, const void* x, float* out, void* workspace, long workspace_bytes, int N, long V, int C, float scale,
                  bts_stream_t stream);
/* out = res * (sigmoid(res . w_sp) + ch[n]) + relu(GN2(c2))   (resnet.py:127-137) */
/* sp_out (may be NULL): the per-voxel spatial gate sigmoid(res . w_sp), fp32 [N*V], kept for the backward pass */
int bts_lp_block_epilogue(int dtype, const void* res, const void* c2, void* out, float* sp_out, const float* wsp, const float* ch, const float* gamma,
                          const float* beta, const float* mean, const float* rstd, int N, long V, int C, int ldo, int G, int mode,
                          bts_stream_t stream);
/* The FIRST ResnetBlock's two convolutions of the raw in_ch = 2 volume in a forward without a backward (resnet.py:30-37,80-87,118 at encoder
 * level 0; model.py:63-68): c1 = conv3x3x3(x) + b3 and res = conv1x1x1(x) + b1 in the storage type (dense, F channels) from ONE pass over the
 * fp32 input x (N,D,H,W,2), GroupNorm-1's BTS_GN_SLAB statistics of c1 (mean, rstd [N*G]) and gap[n][c] = mean over voxels of res (the
 * gate's squeeze, resnet.py:121).  w3 (3,3,3,2,F), w1 (1,1,1,2,F): the reference's fp32 kernels, unpacked.  Replaces bts_lp_cast_pad16 +
 * bts_lp_conv1_gap + bts_lp_conv3d_fwd_gn on the zero-padded 16-channel copy.  Workspace query -1 / BTS_ERR_UNSUPPORTED outside its shapes
 * (F in {8,16,24,32}, D % G == 0, F % G == 0). */
long bts_lp_first_block_workspace(int N, int D, int H, int W, int F, int G);
int bts_lp_first_block_fwd(int dtype, const float* x, const float* w3, const float* b3, const float* w1, const float* b1, void* c1, void* res,
                           float* mean, float* rstd, float* gap, void* workspace, long workspace_bytes, int N, int D, int H, int W, int F,
                           int G, float eps, bts_stream_t stream);
/* The last decoder block's epilogue with the output head in it (decoder.py:55-63: Conv3D 1x1x1 -> out_ch, sigmoid; model.py:63-68 in a
 * forward without a backward): y_head [N*V][K] fp32 = sigmoid?(out . head_w + head_b) with `out` as bts_lp_block_epilogue forms it, never
 * written.  head_w (C, K) fp32 row-major, head_b (K) or NULL.  BTS_ERR_UNSUPPORTED outside the fused kernel's shapes (K <= 4, C <= 64,
 * whole 2048-element chunks per unit): call bts_lp_block_epilogue and bts_lp_head. */
int bts_lp_block_epilogue_head(int dtype, const void* res, const void* c2, float* y_head, const float* wsp, const float* ch, const float* gamma,
                               const float* beta, const float* mean, const float* rstd, const float* head_w, const float* head_b, int N,
                               long V, int C, int G, int mode, int K, int sigmoid, bts_stream_t stream);
/* y = conv3x3x3(x) + bias in the storage type (dense) and the BTS_GN_SLAB statistics of y (resnet.py:80-93 conv -> GroupNormalization)
 * in one pass where the tiled kernel can emit the partial sums from its epilogue; the 16-bit counterpart of bts_conv3d_fwd_gn */
long bts_lp_conv3d_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int G);
int bts_lp_conv3d_fwd_gn(int dtype, const void* x, const void* wp, const float* bias, void* y, float* mean, float* rstd, void* workspace,
                         long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int G, float eps,
                         bts_stream_t stream);
/* conv1 AND the shortcut of a ResnetBlock from ONE pass over the block input (resnet.py:118 and resnet.py:134 read the same `inputs`):
 * y = conv3x3x3(x) + bias with GroupNorm G's statistics of y (as bts_lp_conv3d_fwd_gn), res = conv1x1x1(x) + bias_pt and gap[n][c] = mean
 * over the voxels of the unrounded res (as bts_lp_conv1_gap).  The shortcut is a second set of output columns at the centre tap of the
 * z-marching kernel's input planes: x is read once.  wp / wp_pt = bts_lp_pack(K3S1 / K1, BTS_ROLE_FWD, ...) with the same Cin_slab and
 * fold; y, res dense (N,D,H,W,Cout).  Cin = 64 on volumes of >= 8 M voxels: both ride on the two z-marching passes over the channel halves.
 * x_split (elements; 0 = x is one (N,D,H,W,Cin) view): Cin = 64 as TWO 32-channel tensors x and x + x_split with voxel stride ldx each -- the
 * operands of a concat (decoder.py:75) never materialised side by side, each read in whole lines (virtual concat as a list of
 * (ptr, C) segments); the two passes at any volume size (pass ldx = 32 to the workspace query).  Workspace query -1 / return value 1 (nothing
 * launched) outside the kernel's shapes: run bts_lp_conv1_gap +
 * bts_lp_conv3d_fwd_gn.  BTS_LP_FS=0 in the environment: never (A/B aid) */
long bts_lp_conv3d_fwd_gn_shortcut_workspace(int N, int D, int H, int W, int Cin, int ldx, int Cout, int G);
int bts_lp_conv3d_fwd_gn_shortcut(int dtype, const void* x, long x_split, const void* wp, const float* bias, void* y, float* mean, float* rstd,
                                  const void* wp_pt, const float* bias_pt, void* res, float* gap, void* workspace, long workspace_bytes,
                                  int N, int D, int H, int W, int Cin, int ldx, int Cout, int G, float eps, bts_stream_t stream);
/* The same with the GroupNorm + ReLU of the INPUT applied on the way in (in_relu = 1): y = conv3x3x3(relu(GN_in(x))) + bias and the statistics of y.
 * conv2 of a ResnetBlock reading conv1's raw output (layers/resnet.py:133-136: conv -> GroupNormalization -> relu -> conv) in a forward
 * whose normalised tensor nobody else reads (Model.call(inference=True), model.py:58-71; test.py:128-151): the separate apply pass of
 * layers/group_norm.py:110-122 goes away.  x dense (N,D,H,W,Cin); in_* = that GroupNorm's parameters and statistics (slab mode).
 * The workspace query returns -1 and the call BTS_ERR_UNSUPPORTED where no kernel takes the shape in this form. */
long bts_lp_conv3d_gnin_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int in_G, int G);
int bts_lp_conv3d_gnin_fwd_gn(int dtype, const void* x, const float* in_gamma, const float* in_beta, const float* in_mean,
                              const float* in_rstd, int in_G, int in_relu, const void* wp, const float* bias, void* y, float* mean,
                              float* rstd, void* workspace, long workspace_bytes, int N, int D, int H, int W, int Cin, int Cout, int G,
                              float eps, bts_stream_t stream);
/* The same idea for TRAINING: conv2's weight gradient dW[t][c][k] = sum_v a[v + off_t][c] dy[v][k], a = relu(GN_in(x)), taken from the RAW x
 * (the streaming weight-gradient kernel normalises its planes in LDS) -- with bts_lp_conv3d_gnin_fwd_gn in the forward, relu(GN1(c1)) of
 * layers/resnet.py:133-134 is never written (what tf.GradientTape keeps alive for train.py:151 is c1 alone).
 * bts_lp_conv3d_gnin_train_ok: 1 when both kernels take the shape in this form (ask before the forward), 0 otherwise (not a status).
 * bts_lp_conv3d_gnin_bwd_weight: x dense (N,D,H,W,Cin) raw; dy rows of lddy; dw (3,3,3,Cin,Cout) fp32 (+)=; db (may be NULL) (+)=;
 * workspace of bts_lp_conv3d_bwd_weight_workspace(BTS_CONV_K3S1, ...). */
int bts_lp_conv3d_gnin_train_ok(int N, int D, int H, int W, int Cin, int Cout, int in_G, int G);
int bts_lp_conv3d_gnin_bwd_weight(int dtype, const void* x, const float* in_gamma, const float* in_beta, const float* in_mean,
                                  const float* in_rstd, int in_G, const void* dy, float* dw, float* db, void* workspace,
                                  long workspace_bytes, int N, int D, int H, int W, int Cin, int Cout, int lddy, int accumulate,
                                  bts_stream_t stream);
/* y = Conv3DTranspose(k3, s2, 'same')(x) + bias (dense fine tensor (N,2D,2H,2W,Cout), storage type) and the slab-mode GroupNorm
 * statistics of y in one pass: ConvUpsample (upsample.py:28-43: conv -> GroupNormalization) without a statistics pass over the fine
 * tensor.  (D,H,W): the COARSE grid; wp = bts_lp_pack(BTS_CONV_K3S2T, BTS_ROLE_FWD, ...).  Falls back to the conv + bts_lp_gn_stats
 * where the merged transposed-conv kernel does not take the call or a group is not whole fine planes. */
long bts_lp_convT3d_fwd_gn_workspace(int N, int D, int H, int W, int Cin, int Cout, int G);
int bts_lp_convT3d_fwd_gn(int dtype, const void* x, const void* wp, const float* bias, void* y, float* mean, float* rstd, void* workspace,
                          long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int G, float eps,
                          bts_stream_t stream);
/* res = conv1x1x1(x) + bias in the storage type (dense, ldres == Cout) and gap[n][c] = mean over voxels of res: the block's
 * shortcut and the squeeze of its gate (resnet.py:118-121) in one pass (column sums from the conv epilogue + a small finalize) */
long bts_lp_conv1_gap_workspace(int N, long V, int Cout);
int bts_lp_conv1_gap(int dtype, const void* x, const void* wp, const float* bias, void* res, float* gap, void* workspace,
                     long workspace_bytes, int N, int D, int H, int W, int Cin, int ldx, int Cout, int ldres, bts_stream_t stream);
/* gate backward (resnet.py:121-130 under autodiff) on 16-bit dout / res -> dres in the storage type; fp32 parameter gradients;
 * sp = the sp_out of bts_lp_block_epilogue; ds [N*V] and dgap [N*F] are fp32 scratch outputs; dbias (may be NULL, F floats, += when
 * accumulate_params): column sums of dres = the bias gradient of the block's 1x1x1 shortcut conv (resnet.py:96-103) */
long bts_lp_se_bwd_workspace(int N, long V, int F, int R);
int bts_lp_se_bwd(int dtype, const void* dout, const void* res, const float* sp, const float* gap, const float* h, const float* ch,
                  const float* w1, const float* w2, const float* wsp, void* dres, float* ds, float* dgap, float* dw1, float* dw2, float* dwsp,
                  void* workspace, long workspace_bytes, int N, long V, int F, int R, int lddo, int accumulate_params, float* dbias,
                  bts_stream_t stream);
/* A ResnetBlock's gate backward and GroupNorm-2 (+ReLU) backward in one pair of passes (resnet.py:121-137 under TF autodiff): what
 * bts_lp_se_bwd followed by bts_lp_gn_bwd compute, reading the block-output gradient dout (N,V,F; rows of lddo) twice instead of four
 * times.  res, c2 dense; dres, dc2 dense outputs in the storage type; ds (N*V) / dgap (N,F) fp32 scratch outputs; parameter gradients
 * accumulate; dbias_pt / dbias_c2 (may be NULL): bias gradients of the shortcut conv / conv2 (+=).  BTS_ERR_UNSUPPORTED outside the
 * kernels' tiling (the caller runs the two separate entry points). */
long bts_lp_block_bwd_workspace(int N, long V, int F, int R, int G);
int bts_lp_block_bwd(int dtype, const void* dout, int lddo, const void* res, const void* c2, const float* sp, const float* gap, const float* h,
                     const float* ch, const float* w1, const float* w2, const float* wsp, const float* gamma, const float* beta,
                     const float* mean, const float* rstd, void* dres, void* dc2, float* ds, float* dgap, float* dw1, float* dw2, float* dwsp,
                     float* dgamma, float* dbeta, float* dbias_pt, float* dbias_c2, void* workspace, long workspace_bytes, int N, long V, int F,
                     int R, int G, bts_stream_t stream);
/* All 16-bit weight images in one launch (they go stale together at the optimiser step, train.py:152): host table of
 * bts_lp_pack_desc_bytes()-sized descriptors filled by bts_lp_pack_desc (arguments as bts_lp_pack; returns the entry's block count > 0 or
 * a negative engine code; first_block = running sum of those counts), copied to device memory by the caller. */
long bts_lp_pack_desc_bytes(void);
long bts_lp_pack_desc(void* host_table, int index, long first_block, int kind, int role, const float* w, void* wp, int Cin_ref, int Cout,
                      int Cin_slab, int dup_start, int dup_shift);
int bts_lp_pack_batch(int dtype, const void* table_dev, int n, long total_blocks, bts_stream_t stream);
/* the non-default samplers on 16-bit tensors (args.py:136-141): MaxPooling3D(2) (downsample.py:51-70; (D,H,W) = INPUT dims, idx the
 * window position of the first maximum per output element, NULL when no gradient is wanted) and UpSampling3D(2) (upsample.py:69;
 * (D,H,W) = COARSE dims), with their gradients; C % 8 == 0, channel-slice views allowed */
int bts_lp_maxpool2_fwd(int dtype, const void* x, void* y, uint8_t* idx, int N, int D, int H, int W, int C, int ldx, int ldy,
                        bts_stream_t stream);
int bts_lp_maxpool2_bwd(int dtype, const void* dy, const uint8_t* idx, void* dx, int N, int D, int H, int W, int C, int lddy, int lddx,
                        int accumulate, bts_stream_t stream);
int bts_lp_upsample2_fwd(int dtype, const void* x, void* y, int N, int D, int H, int W, int C, int ldx, int ldy, bts_stream_t stream);
int bts_lp_upsample2_bwd(int dtype, const void* dy, void* dx, int N, int D, int H, int W, int C, int lddy, int lddx, int accumulate,
                         bts_stream_t stream);
/* output head (decoder.py:55-63): y = sigmoid(x . W + b), W (C, K <= 4) fp32, y fp32 (the label map is taken from it); x rows of
 * ldx >= C elements, C > 0, C % 8 == 0 and ldx % 8 == 0 (BTS_ERR_SHAPE otherwise) */
int bts_lp_head(int dtype, const void* x, const float* w, const float* bias, float* y, long nvox, int C, int ldx, int K, int sigmoid,
                bts_stream_t stream);
/* output head backward (decoder.py:55-63 under autodiff; train.py:142-151): dpre = dL/d(x . W + b) (nvox, K) fp32 (bts_sigmoid_bwd) ->
 * dx (nvox, C) in the storage type, dw (C, K) and db (K) fp32 (+= when accumulate), all from ONE pass over x.  C in {16,32,64}, K <= 4 */
long bts_lp_head_bwd_workspace(int C, int K);
int bts_lp_head_bwd(int dtype, const void* x, const float* dpre, const float* w, void* dx, float* dw, float* db, void* workspace,
                    long workspace_bytes, long nvox, int C, int ldx, int lddx, int K, int accumulate, bts_stream_t stream);

/* ---- data-parallel exchange over RCCL on device buffers (the reference is single-device, train.py:138) --------------------
 * Sharding train.py:140-152 by sample needs three collectives: C1 the sum of the flat fp32 gradient buffer over the ranks (in a few
 * large buckets: xGMI is point to point, a ring is per-link bound, few large messages win), C2 rank `root`'s parameters on every rank
 * after initialisation / load, C3 the sum of the raw loss sums (bts_loss_sums) and of the Dice table, which the reference sums over the
 * batch axis (util.py:11,18-20).  comm = the caller's ncclComm_t (one process per GPU); every call is enqueued on `stream` and returns
 * BTS_OK, a BTS_ERR_* code, or BTS_ERR_RCCL_BASE - ncclResult_t.  RCCL is bound on first use by dlopen (the copy the process already holds,
 * else the system one): the library has no link-time dependency on it; bts_dp_available says whether it was found (BTS_ERR_UNSUPPORTED
 * from the others when not).  bts_dp_comm_* are conveniences over ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy for hosts that do
 * not link RCCL themselves (unique id: bts_dp_unique_id_bytes() bytes, made on one rank and handed to the others by the host's own means).
 * bts_amd.parallel issues the same three collectives through torch.distributed, whose 'nccl' backend is RCCL. */
int bts_dp_available(void);
long bts_dp_unique_id_bytes(void);
int bts_dp_comm_unique_id(void* id_out);
int bts_dp_comm_init(void** comm_out, int nranks, const void* id, int rank);
int bts_dp_comm_destroy(void* comm);
/* C1: in-place sum over the ranks of the buckets [bucket_off[b], bucket_off[b] + bucket_len[b]) (elements; host arrays) of the flat
 * gradient buffer, one RCCL group per call.  Call it once per finished bucket from inside the backward for the overlapped form. */
int bts_dp_allreduce_buckets(void* comm, float* flat_grads, const long* bucket_off, const long* bucket_len, int nbuckets, bts_stream_t stream);
/* C2 */
int bts_dp_broadcast_params(void* comm, float* flat_params, long n, int root, bts_stream_t stream);
/* C3: in-place sum of n fp64 values */
int bts_dp_allreduce_small(void* comm, double* sums, int n, bts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BTS_HIP_H */
