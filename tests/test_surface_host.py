"""CPU: the NumPy restatement of the distance side of the score (tests/surface_ref.py) against SciPy and brute force,
infer.region_rates_from_confusion, the --surface_metrics flag and the argument validation of the entry points of csrc/surface.hip.
No kernel runs here; the device side is tests/test_surface_gpu.py."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import segment_ref as S  # noqa: E402
import surface_ref as H  # noqa: E402

import bts_amd  # noqa: E402,F401
from bts_amd import infer  # noqa: E402
from bts_amd import test as T  # noqa: E402

SHAPES = [(5, 6, 7), (1, 9, 70), (17, 3, 300), (33, 70, 65)]
SPACINGS = [(1.0, 1.0, 1.0), H.widened((1.2, 1.0, 0.9))]


def features(shape, seed):
    f = (np.random.default_rng(seed).random(shape) < 0.01).astype(np.uint8)
    f[-1, -1, -1] = 1
    return f


@pytest.mark.parametrize('spacing', SPACINGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_against_scipy(shape, spacing):
    ndi = pytest.importorskip('scipy.ndimage')
    f = features(shape, 3)
    ref = ndi.distance_transform_edt(f == 0, sampling=spacing)
    got = np.sqrt(H.edt_sq(f, spacing))
    assert np.all(np.abs(got - ref) <= 1e-12 * ref)


@pytest.mark.parametrize('spacing', SPACINGS)
def test_restatement_against_brute_force(spacing):
    f = features((5, 6, 7), 4)
    f[1, 2, 3] = 1
    ref = H.edt_sq_brute(f, spacing)
    got = H.edt_sq(f, spacing)
    assert np.all(np.abs(got - ref) <= 1e-12 * ref)
    assert np.all(np.isinf(H.edt_sq(np.zeros((3, 4, 5), np.uint8), spacing)))


def test_surface_definition_equals_scipy_erosion():
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(5)
    st = ndi.generate_binary_structure(3, 1)
    for shape in SHAPES + [(1, 1, 1), (4, 1, 3)]:
        for density in (0.2, 0.9, 1.0, 0.0):
            a = rng.random(shape) < density
            assert np.array_equal(H.surface(a), a & ~ndi.binary_erosion(a, st, border_value=0)), (shape, density)


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=1e-14, abs=0.0)


def test_region_rates_equal_the_onehot_arithmetic():
    rng = np.random.default_rng(7)
    lab = np.array([0, 1, 2, 4], dtype=np.uint8)
    truth = lab[rng.integers(0, 4, size=(9, 7, 5))]
    pred = np.where(rng.random(truth.shape) < 0.7, truth, lab[rng.integers(0, 4, size=truth.shape)]).astype(np.uint8)
    cases = [(truth, pred), (truth, truth), (np.zeros_like(truth), pred), (truth, np.zeros_like(truth)),
             (np.full_like(truth, 4), np.full_like(truth, 4)), (np.where(truth == 4, 0, truth), np.where(pred == 4, 0, pred))]
    for t, p in cases:
        got = infer.region_rates_from_confusion(S.confusion(t, p, 4))
        assert set(got) == {'sens_wt', 'sens_tc', 'sens_et', 'spec_wt', 'spec_tc', 'spec_et'}
        for name, cm in H.BRATS.items():
            sens, spec = H.rates_onehot(t, p, cm)
            assert same(got['sens_' + name], sens) and same(got['spec_' + name], spec), name
    assert math.isnan(infer.region_rates_from_confusion(S.confusion(cases[2][0], cases[2][1], 4))['sens_wt'])      # no truth voxel
    assert math.isnan(infer.region_rates_from_confusion(S.confusion(cases[4][0], cases[4][1], 4))['spec_wt'])      # no background
    with pytest.raises(ValueError, match='4 x 4'):
        infer.region_rates_from_confusion(np.zeros((3, 3)))
    # scores_from_confusion keeps its keys
    assert set(infer.scores_from_confusion(S.confusion(truth, pred, 4))) == {'confusion', 'macro', 'micro', 'dice', 'wt', 'tc', 'et'}


def test_entry_points_validate_before_any_hip_call():
    """BTS_ERR_SHAPE (-1) with NULL pointers and no GPU; nothing to do returns 0 without a launch"""
    from bts_amd._lib import lib
    L = lib()

    def surf(d=4, h=5, w=6, k=4, cm=14):
        return L._bts_region_surface(None, None, None, d, h, w, k, cm, None)

    for name in ('d', 'h', 'w'):
        assert surf(**{name: 0}) == -1 and surf(**{name: -3}) == -1, name
    for k in (-1, 0, 1, 9, 64):
        assert surf(k=k) == -1, k
    assert surf(cm=-1) == -1 and surf(cm=16) == -1 and surf(k=2, cm=4) == -1

    def edt(d=4, h=5, w=6, sd=1.0, sh=1.0, sw=1.0):
        return L._bts_edt3d_sq(None, None, d, h, w, sd, sh, sw, None)

    for name in ('d', 'h', 'w'):
        assert edt(**{name: 0}) == -1 and edt(**{name: -3}) == -1, name
    for name in ('sd', 'sh', 'sw'):
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            assert edt(**{name: bad}) == -1, (name, bad)

    ranks = (ctypes.c_long * 8)(0, 1, 2, 3, 4, 5, 6, 7)
    rp = ctypes.cast(ranks, ctypes.c_void_p)

    def sel(n=10, nranks=3, r=rp):
        return L._bts_masked_select(None, None, n, r, nranks, None, None, None)

    assert sel(n=-1) == -1 and sel(nranks=-1) == -1 and sel(nranks=9) == -1
    bad = (ctypes.c_long * 3)(0, -1, 2)
    assert sel(r=ctypes.cast(bad, ctypes.c_void_p)) == -1
    assert sel(n=0) == 0 and sel(nranks=0) == 0                              # nothing to do, nothing launched
    for nr in range(1, 9):
        assert L._bts_masked_select_workspace(nr) > 0
    assert L._bts_masked_select_workspace(0) < 0 and L._bts_masked_select_workspace(9) < 0


def test_the_flag_parses_and_defaults_to_off():
    required = ['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--tumor_prepro', 'p.npy', '--tumor_model', 'm']
    assert T.parse_args(required).surface_metrics is False
    assert T.parse_args(required + ['--surface_metrics']).surface_metrics is True
    assert T.SURFACE_KEYS == ('hd95_wt', 'hd95_tc', 'hd95_et', 'sens_wt', 'sens_tc', 'sens_et', 'spec_wt', 'spec_tc', 'spec_et')
    assert math.isnan(T.mean_finite([float('inf'), float('nan')])) and T.mean_finite([1.0, float('inf'), 3.0]) == 2.0
