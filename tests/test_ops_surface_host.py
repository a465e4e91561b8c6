"""The surface of the `ops` package, checked without a GPU: every name callers use still resolves on `ops`, each is defined in exactly one
subject module, no subject module holds a binding of its own of what tests swap in `ops._core`, and one wrapper per subject module turns a
bad tensor away -- with the exception type callers have always seen -- before the library is reached."""
import sys

import pytest
import torch

# the public names of ops.py at the commit before it became a package (sorted(vars(ops)) without the private names and the imported modules)
PUBLIC = """
ERRORS FLAG_ACCUM FLAG_SIGMOID GN_CHANNEL GN_SLAB INTENSITY_BLUR INTENSITY_BRIGHT INTENSITY_CONTRAST INTENSITY_GAMMA INTENSITY_INVERT
INTENSITY_NOISE K1 K3S1 K3S2 K3S2T N4_MAX_AXIS N4_MAX_BINS N4_MAX_MESH PackTable REGION_CHANNELS ROLE_BWD ROLE_FWD adam_tf_step
add_strided affine_resample3d augment_batch augment_batch_max augment_crop augment_spatial_batch augment_spatial_batch_max axpy
block_bwd block_bwd_takes block_epilogue_fwd case_norm channel_moments check_clip colsum component_boxes component_largest
component_sizes components3d components_apply conv_bwd_data conv_bwd_data_pair conv_bwd_weight conv_bwd_weight_form
conv_bwd_weight_kernel conv_flops conv_fwd conv_fwd_fused2 conv_fwd_fused2_gn conv_fwd_gn conv_kind_taps conv_out_shape conv_pack
conv_packed_empty dense_bwd dense_fwd dice_metric_sums dice_metric_value dilate3d dropout_apply dropout_mask edt3d_sq
enable_side_streams fill flip_affine gn_apply gn_bwd gn_stats grad_nonfinite intensity_batch intensity_blur_weights join_side_stream
joint_hist_pv kernel_symbol l2_reg_bwd l2_reg_fwd label_confusion ld_of lesion_crop lesion_pairs lesion_pairs_capacity lib loss_bwd
loss_sums loss_value masked_select maxpool2_bwd maxpool2_fwd n4_apply n4_eval n4_fit n4_hist n4_lattice n4_log_lattice n4_residual
normal prepro_crop_norm prepro_occupancy prepro_sums profile_enable profile_records quantize_bins region_dice_sums region_finish
region_relabel region_surface region_targets relu_bwd reorient3d scalar_lincomb se_bwd se_mlp_fwd seg_loss_bwd seg_loss_sums
seg_loss_value side_stream sigmoid_bwd skull_strip spline_prefilter3d step_fence step_fence_done tta_finish upsample2_bwd upsample2_fwd
vae_sample_bwd vae_sample_fwd wait_side_stream_event window_accumulate window_batch_max window_gather window_occupancy workspace zoom3d
""".split()
PRIVATE = ('_p', '_stream', '_fence', '_check')                  # private names that code outside the package reads as ops.NAME
SUBJECTS = ('_core', 'streams', 'profile', 'conv', 'norm', 'pointwise', 'loss', 'volume', 'window', 'score', 'augment', 'regions', 'prepro',
            'coreg', 'n4')
SWAPPED = ('workspace', '_check', '_p', '_stream', 'lib')          # what tests replace in ops._core: reached as _core.NAME only


def ops():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops


def subjects():
    o = ops()
    return {name: getattr(o, name) for name in SUBJECTS}


def test_every_name_of_the_former_module_resolves():
    o = ops()
    assert len(PUBLIC) == len(set(PUBLIC)) == 136
    missing = [n for n in PUBLIC + list(PRIVATE) if not hasattr(o, n)]
    assert not missing, missing


def test_each_name_is_defined_in_one_subject_module_and_ops_holds_that_object():
    o, mods = ops(), subjects()
    for name in PUBLIC + list(PRIVATE):
        obj = getattr(o, name)
        if callable(obj):                                              # functions and PackTable say where they were defined
            home = obj.__module__.rsplit('.', 1)[-1]
            home = '_core' if home == '_lib' else home               # (lib itself comes from _lib, through _core)
            owners = [home]
        else:                                                          # constants and the state dicts: the modules that hold the name
            owners = [m for m in SUBJECTS if name in vars(mods[m])]
        assert len(owners) == 1 and owners[0] in SUBJECTS, (name, owners)
        assert getattr(mods[owners[0]], name) is obj, name
    defined = {}
    for m, mod in mods.items():
        for name, obj in vars(mod).items():
            if callable(obj) and getattr(obj, '__module__', None) == mod.__name__:
                defined.setdefault(name, []).append(m)
    twice = {n: ms for n, ms in defined.items() if len(ms) > 1}
    assert not twice, twice


def test_state_exists_once():
    o, mods = ops(), subjects()
    assert o._fence is mods['streams']._fence
    for name, home in (('_workspaces', '_core'), ('_side', 'streams'), ('_fence', 'streams'), ('_side_enabled', 'streams')):
        assert [m for m in SUBJECTS if name in vars(mods[m])] == [home], name


def test_no_subject_module_binds_what_tests_swap_in_core():
    mods = subjects()
    for m in SUBJECTS[1:]:
        held = [n for n in SWAPPED if n in vars(mods[m])]
        assert not held, (m, held)
        assert vars(mods[m]).get('_core', mods['_core']) is mods['_core'], m
    loaded = [n for n in sys.modules if n.startswith('bts_amd.ops.')]
    assert sorted(loaded) == sorted('bts_amd.ops.' + m for m in SUBJECTS), loaded      # __init__ imports every one, eagerly


def test_the_swapped_names_have_one_binding_seen_from_both_sides(monkeypatch):
    """ops.NAME reads and assigns ops._core.NAME: a swap made in _core, as tests/guard_alloc.py makes it, is what a caller of ops.NAME outside
    the package gets (lowp.py calls ops.workspace), and a swap made on ops, as a helper written against the single file makes it, is what
    the wrappers get; either is undone in both"""
    import guard_alloc
    from bts_amd import lowp
    o = ops()
    assert lowp.ops is o
    for name in SWAPPED:
        assert name not in vars(o), name
        real = getattr(o._core, name)
        for target in (o._core, o):
            with monkeypatch.context() as mp:
                stand_in = object()
                mp.setattr(target, name, stand_in)
                assert getattr(o._core, name) is stand_in and getattr(lowp.ops, name) is stand_in, (name, target.__name__)
            assert getattr(o._core, name) is real and getattr(o, name) is real, (name, target.__name__)
    real = o._core.workspace
    with monkeypatch.context() as mp:
        guard_alloc.install(mp)
        buf = lowp.ops.workspace(24, torch.device('cpu'))              # the lookup lowp.py makes
        assert buf.numel() == 24 and bool((buf == guard_alloc.FILL).all())      # exact size, filled: not the 1 MB grow-only buffer
        assert o._core.workspace is o.workspace
    assert o.workspace is o._core.workspace is real


class OnGpu(torch.Tensor):
    """a CPU tensor that says it lives on the GPU: the stand-in that lets the dtype, layout and rank rules be reached without a device"""
    is_cuda = property(lambda self: True)


def bad(kind, shape, dtype):
    """a tensor that breaks one clause of 'a dense `dtype` tensor of this rank on the GPU' ('ok': none)"""
    if kind == 'cpu':
        return torch.zeros(shape, dtype=dtype)
    if kind == 'dtype':
        return torch.zeros(shape, dtype=torch.float64 if dtype != torch.float64 else torch.float32).as_subclass(OnGpu)
    if kind == 'strided':
        return torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype).as_subclass(OnGpu)[..., ::2]
    if kind == 'rank':
        return torch.zeros(shape[1:], dtype=dtype).as_subclass(OnGpu)
    return torch.zeros(shape, dtype=dtype).as_subclass(OnGpu)


u8, f32, f64 = torch.uint8, torch.float32, torch.float64
# wrapper: (good shape, dtype, call, what ops.py raised for a tensor (on the CPU, of another dtype, strided, of one dimension fewer))
# as recorded from the module this package replaced; None: that wrapper takes such a tensor (conv_pack copies a strided kernel and leaves
# the rank to the library, quantize_bins is element-wise)
REJECT = {
    'edt3d_sq': ((4, 5, 6), u8, lambda o, t: o.edt3d_sq(t), (ValueError, ValueError, ValueError, ValueError)),
    'components3d': ((4, 5, 6), u8, lambda o, t: o.components3d(t, 14), (ValueError, ValueError, ValueError, ValueError)),
    'dilate3d': ((4, 5, 6), u8, lambda o, t: o.dilate3d(t, 14), (ValueError, ValueError, ValueError, ValueError)),
    'zoom3d': ((4, 5, 6, 2), f32, lambda o, t: o.zoom3d(t, (8, 8, 8)), (RuntimeError, RuntimeError, ValueError, ValueError)),
    'window_occupancy': ((4, 5, 6, 1), f32, lambda o, t: o.window_occupancy(t, (2, 2, 2), ([0, 2], [0, 3], [0, 4])),
                         (RuntimeError, RuntimeError, ValueError, ValueError)),
    'prepro_sums': ((4, 5, 6, 2), f32, lambda o, t: o.prepro_sums(t, bad('ok', (4,), f64)), (ValueError, ValueError, ValueError, ValueError)),
    'quantize_bins': ((4, 5, 6), f32, lambda o, t: o.quantize_bins(t, 0.0, 1.0), (ValueError, ValueError, ValueError, None)),
    'n4_log_lattice': ((4, 5, 6), f32, lambda o, t: o.n4_log_lattice(t), (ValueError, ValueError, ValueError, ValueError)),
    'case_norm': ((4, 5, 6, 2), f32, lambda o, t: o.case_norm(t), (ValueError, ValueError, ValueError, ValueError)),
    'region_targets': ((2, 3), f32, lambda o, t: o.region_targets(t), (ValueError, ValueError, ValueError, ValueError)),
    'conv_pack': ((3, 3, 3, 4, 8), f32, lambda o, t: o.conv_pack(o.K3S1, o.ROLE_FWD, t, 4, 8), (RuntimeError, RuntimeError, None, None)),
}


class Reached(Exception):
    pass


@pytest.mark.parametrize('name', sorted(REJECT))
def test_a_wrapper_of_each_subject_refuses_a_bad_tensor_before_the_library(name, monkeypatch):
    o = ops()

    def reached():
        raise Reached()
    monkeypatch.setattr(o._core, 'lib', reached)
    shape, dtype, call, expected = REJECT[name]
    for kind, exc in zip(('cpu', 'dtype', 'strided', 'rank'), expected):
        if exc is None:
            continue
        with pytest.raises(exc) as info:
            call(o, bad(kind, shape, dtype))
        assert info.type is exc, (name, kind, info.type)               # RuntimeError where it was one, ValueError where it was one
    with pytest.raises(Reached):                                       # ... and the good tensor gets as far as the library
        call(o, bad('ok', shape, dtype))
