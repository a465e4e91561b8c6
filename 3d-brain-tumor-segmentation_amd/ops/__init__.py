"""Thin, checked Python wrappers over the C ABI (include/bts_hip.h): torch tensors in, raw pointers out.

torch is used for device memory and the current HIP stream only.  Every function enqueues on
torch.cuda.current_stream() and raises RuntimeError on a non-zero status -- there is no CPU path.
Activations are [N,D,H,W,C] fp32 tensors whose last-dim stride is 1 and whose voxel stride (`ld`) may exceed C
(channel slices of a slab).

One module per subject, named for the csrc/ file it binds where there is one; `_core` holds what they share.  Every subject module is
imported here, eagerly, and its names re-exported: `ops.NAME` is the public surface, and a test that swaps `torch` in every loaded module
(tests/guard_alloc.py) reaches all of them.  State lives once, in the module that owns it (`_core._workspaces`, `streams._side`,
`streams._fence`): read `ops._fence` as the same dict, but rebind nothing here.

The five names the wrappers look up in `_core` at call time (`lib`, `workspace`, `_check`, `_p`, `_stream`) are bound THERE and nowhere
else: `ops.NAME` is a property that reads and assigns `_core.NAME`.  Code outside the package calls `ops.workspace(...)` (lowp.py) and
`ops._p(...)`; with a second binding here, a test that swaps the workspace in `_core` would miss those callers, and one that swaps it on
`ops` would miss the wrappers.
"""
import sys
import types

from . import _core, streams, profile, conv, norm, pointwise, loss, volume, window, score, augment, regions, prepro, coreg, n4      # noqa: F401
from ._core import (ERRORS, FLAG_ACCUM, FLAG_SIGMOID, GN_CHANNEL, GN_SLAB, K1, K3S1, K3S2, K3S2T, ROLE_BWD, ROLE_FWD, ld_of)      # noqa: F401
from .streams import (_fence, enable_side_streams, join_side_stream, side_stream, step_fence, step_fence_done,      # noqa: F401
                      wait_side_stream_event)
from .profile import conv_flops, kernel_symbol, profile_enable, profile_records      # noqa: F401
from .conv import (PackTable, conv_bwd_data, conv_bwd_data_pair, conv_bwd_weight, conv_bwd_weight_form, conv_bwd_weight_kernel,      # noqa: F401
                   conv_fwd, conv_fwd_fused2, conv_fwd_fused2_gn, conv_fwd_gn, conv_kind_taps, conv_out_shape, conv_pack, conv_packed_empty)
from .norm import block_bwd, block_bwd_takes, block_epilogue_fwd, colsum, gn_apply, gn_bwd, gn_stats, se_bwd, se_mlp_fwd      # noqa: F401
from .pointwise import (add_strided, axpy, dense_bwd, dense_fwd, dropout_apply, dropout_mask, fill, maxpool2_bwd, maxpool2_fwd,      # noqa: F401
                        normal, relu_bwd, scalar_lincomb, sigmoid_bwd, upsample2_bwd, upsample2_fwd, vae_sample_bwd, vae_sample_fwd)
from .loss import (adam_tf_step, dice_metric_sums, dice_metric_value, grad_nonfinite, l2_reg_bwd, l2_reg_fwd, loss_bwd, loss_sums,      # noqa: F401
                   loss_value, seg_loss_bwd, seg_loss_sums, seg_loss_value)
from .volume import (UNCERTAINTY_MODES, affine_resample3d, ensemble_update, flip_affine, label_resample3d, reorient3d, skull_strip,      # noqa: F401
                     spline_prefilter3d, tta_finish, uncertainty_finish, zoom3d)
from .window import window_accumulate, window_batch_max, window_gather, window_occupancy      # noqa: F401
from .score import (UNCERTAINTY_LEVELS, component_boxes, component_largest, component_sizes, components3d, components_apply, dilate3d, edt3d_sq,      # noqa: F401
                    label_confusion, lesion_crop, lesion_pairs, lesion_pairs_capacity, masked_select, region_relabel, region_surface,
                    uncertainty_confusion)
from .augment import (CLASS_LOCATIONS_MAX_CLASSES, INTENSITY_BLUR, INTENSITY_BRIGHT, INTENSITY_CONTRAST, INTENSITY_GAMMA, INTENSITY_INVERT, INTENSITY_NOISE,      # noqa: F401
                      augment_batch, augment_batch_max, augment_crop, augment_spatial_batch, augment_spatial_batch_max, channel_moments,
                      class_locations, intensity_batch, intensity_blur_weights)
from .regions import REGION_CHANNELS, region_dice_sums, region_finish, region_targets      # noqa: F401
from .prepro import case_norm, check_clip, prepro_crop_norm, prepro_occupancy, prepro_sums      # noqa: F401
from .coreg import joint_hist_pv, quantize_bins      # noqa: F401
from .n4 import (N4_MAX_AXIS, N4_MAX_BINS, N4_MAX_MESH, n4_apply, n4_eval, n4_fit, n4_hist, n4_lattice, n4_log_lattice,      # noqa: F401
                 n4_residual)


class _Ops(types.ModuleType):
    """this module's type: the names below are properties over `_core`, so each has one binding"""


for _name in ('lib', 'workspace', '_check', '_p', '_stream'):
    setattr(_Ops, _name, property(lambda self, _name=_name: getattr(_core, _name), lambda self, value, _name=_name: setattr(_core, _name, value)))
sys.modules[__name__].__class__ = _Ops
