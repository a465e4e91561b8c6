"""Writes tests/golden/resample_vectors.npz: scipy.ndimage.zoom(mode='reflect') in float64, applied per channel to 3-D arrays (the
oracle of csrc/resample.hip; the GPU tests read only this file and tests/zoom_ref.py, so they need no SciPy).

    python tests/golden/make_resample_golden.py

Inputs are smooth tissue times per-channel intensities up to ~1000 around an exactly-zero region, so the brain mask means something.
Per case the file holds  <name>_x (D,H,W,C) float32,  <name>_y (Do,Ho,Wo,C) float64 (float32 for order 0, whose values are input
samples) and, in `spec`, a JSON list of {name, order, factors | out_shape, pad_res}.  The generator asserts what the tests rely on:
the float64 restatement equals SciPy to 1e-12 * max|ref|, and the float32 restatement alone satisfies the mask criterion of
tests/test_resample_gpu.py (mask differences only where |max_c golden| <= 4 x its own max deviation, on at most 0.1 % of the voxels).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zoom_ref  # noqa: E402

OUT = os.path.join(HERE, 'resample_vectors.npz')

SPEC = [
    # extents 16-40; factors < 1, > 1, exactly 1 and a large one (6.0); C in {1,2,4}; orders 0, 1, 3
    dict(name='cubic_c2_mixed', shape=(16, 16, 18), C=2, order=3, factors=(1.5, 0.6, 1.0)),
    dict(name='cubic_c1_large', shape=(16, 16, 17), C=1, order=3, factors=(0.5, 0.5, 6.0)),
    dict(name='cubic_c4_padmask', shape=(16, 16, 16), C=4, order=3, factors=(1.1, 0.9, 1.0), pad_res=16),
    dict(name='linear_c2', shape=(16, 17, 18), C=2, order=1, factors=(1.3, 0.6, 1.0)),
    dict(name='nearest_c1', shape=(16, 16, 40), C=1, order=0, factors=(1.5, 0.5, 0.7)),
    # the way back: an explicit output extent, here the (20,18,22) scan that pixdim (1.3, 0.9, 0.8) brought to (26,16,18)
    dict(name='cubic_c1_reverse', shape=(26, 16, 18), C=1, order=3, out_shape=(20, 18, 22)),
]


def blob(shape, C, seed):
    """smooth positive tissue times per-channel intensities up to ~1000, with an exactly-zero region of ~25 % of the voxels.
    The zero region is an interior cavity and the faces of the volume carry tissue: an output voxel that coincides with input
    samples (the first and last index of every axis, every index of a factor-1 axis) reproduces them, so where those samples
    are zero its exact value is 0 and its sign is rounding noise in ANY precision, SciPy's float64 included -- such voxels
    would make the golden mask itself arbitrary.  Inside the cavity the spline's ripple is a real, signed value."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    tex = 0.65 + 0.35 * np.sin(4.0 * g[0] + rng.uniform(0, 6)) * np.cos(3.0 * g[1] + rng.uniform(0, 6)) * np.sin(5.0 * g[2] + 1.0)
    chans = []
    for c, a in enumerate(rng.uniform(300.0, 1000.0, C)):
        off = 0.05 * c                                # every modality has its own cavity: the mask is the max over channels
        r2 = ((g[0] - off) / 0.80) ** 2 + (g[1] / 0.78) ** 2 + ((g[2] + off) / 0.80) ** 2
        chans.append(np.where(r2 < 1.0, 0.0, tex * a))
    return np.stack(chans, axis=-1).astype(np.float32)


def out_shape_of(case):
    return tuple(case['out_shape']) if 'out_shape' in case else zoom_ref.zoom_output_shape(case['shape'], case['factors'])


def scipy_per_channel(x, case):
    from scipy.ndimage import zoom
    shape = out_shape_of(case)
    factors = case.get('factors') or tuple(o / n for o, n in zip(shape, x.shape[:3]))
    chans = []
    for c in range(x.shape[-1]):
        y = zoom(x[..., c].astype(np.float64), factors, order=case['order'], mode='reflect')
        assert y.shape == shape, (case['name'], y.shape, shape)
        chans.append(y)
    return np.stack(chans, axis=-1)


def build():
    arrays, spec = {}, []
    for k, case in enumerate(SPEC):
        x = blob(case['shape'], case['C'], seed=100 + k)
        y = scipy_per_channel(x, case)
        shape = out_shape_of(case)
        scale = np.abs(y).max()
        r64 = zoom_ref.zoom(x, shape, case['order'], np.float64)
        assert np.abs(r64 - y).max() <= 1e-12 * scale, (case['name'], np.abs(r64 - y).max() / scale)
        r32 = zoom_ref.zoom(x, shape, case['order'], np.float32)
        tol = 4.0 * np.abs(r32.astype(np.float64) - y).max()
        gm, rm = y.max(axis=-1) > 0, r32.max(axis=-1) > 0
        diff = gm != rm
        assert not np.any(diff & (np.abs(y.max(axis=-1)) > tol)), case['name']
        assert diff.mean() <= 1e-3, (case['name'], diff.mean())
        assert 0.05 < np.mean(x == 0) < 0.6, (case['name'], np.mean(x == 0))
        assert 0.01 < 1.0 - gm.mean() < 0.6, (case['name'], gm.mean())          # the golden mask has both values
        print('%-18s %s -> %s  fp32 restatement: max dev %.3g (%.2g of max|ref|), mask differs on %.4f %%, mask zeros %.1f %%'
              % (case['name'], x.shape, shape, tol / 4, tol / 4 / scale, 100 * diff.mean(), 100 - 100 * gm.mean()))
        arrays[case['name'] + '_x'] = x
        arrays[case['name'] + '_y'] = y.astype(np.float32) if case['order'] == 0 else y
        if case['order'] == 0:
            assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
        spec.append({k2: (list(v) if isinstance(v, tuple) else v) for k2, v in case.items()})
    arrays['spec'] = np.array(json.dumps(spec))
    return arrays


if __name__ == '__main__':
    a = build()
    np.savez_compressed(OUT, **a)
    print('%s: %d bytes' % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= 500 * 1000
