// Internal constants shared by the .hip translation units; the public C ABI is include/bts_hip.h.
#pragma once
#include "../../include/bts_hip.h"

// version.hip: the optional in-library kernel timing -- is it on; events on the launch stream right around the launch of kernel `sym`
int bts_prof_on();
void bts_prof_begin(int sym, double flops, hipStream_t stream);
void bts_prof_end(hipStream_t stream);

// groupnorm.hip: mean / rstd from per-block (sum, sumsq) partials laid out [N*G][B][2] (slab semantics), fixed order
int bts_gn_finalize_partials_(const double* partial, float* mean, float* rstd, int NG, long B, double count, float eps,
                              hipStream_t stream);

// groupnorm.hip, for block_bwd.hip: blocks per (sample, slab) unit / elements per block of the vectorised slab kernels (false: generic shape)
bool bts_gn_slab_blocks_(int N, long V, int C, int G, int* B, long* span);

// se.hip: stage 2 of the gate backward alone (SE-MLP backward from the summed partials red[(n*F+c)*2 + {ch, w}])
int bts_se_mlp_bwd_(const double* red, double* scratch, const float* gap, const float* h, const float* ch, const float* w1, const float* w2,
                    float* dw1, float* dw2, float* dwsp, float* dgap, int N, int B, long V, int F, int R, int accumulate_params,
                    hipStream_t stream);

// conv_igemm.hip: y (+)= act(bias + sum_z part[z][voxel][Npad])  (finish of a split-K launch, fixed summation order); flags: IG_FLAG_*
int bts_igemm_reduce_(const float* part, const float* bias, float* y, long nvox, int Cout, int Npad, int ldy, int ksplit, int flags,
                      hipStream_t stream);
// se.hip: stages 2a + 2 of the gate backward (sum the per-block partials [n][b][F][{ch, w}], SE-MLP backward, dgap / V)
int bts_se_mlp_bwd_sample_(const double* red, double* scratch, const float* h, const float* ch, const float* w1, const float* w2, float* dgap, int N,
                           long V, int F, int R, hipStream_t stream);
int bts_se_bwd_middle_(double* partial, double* red, double* scratch, const float* gap, const float* h, const float* ch, const float* w1,
                       const float* w2, float* dw1, float* dw2, float* dwsp, float* dgap, int N, int B, long V, int F, int R,
                       int accumulate_params, hipStream_t stream);

// conv_pack.hip: the parts of a K3S1 weight image -- implicit GEMM (also read by the small-channel kernels) | F(2x2,3x3) x direct |
// F(2x2x2,3x3x3).  A kernel is about to read part `bit` of the image that starts at `base`: packed on the spot where the last re-pack left
// it out (ensure, before the launch), and recorded once the launch was accepted (mark_used: re-packs then write the parts in use only)
enum : unsigned { IMG_IGEMM = 1u, IMG_WINO = 2u, IMG_W3 = 4u, IMG_ALL = 7u };
int bts_img_ensure_(const float* base, unsigned bit, hipStream_t stream);
void bts_img_mark_used_(const float* base, unsigned bit);
