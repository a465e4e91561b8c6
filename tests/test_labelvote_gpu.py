"""-m gpu: a label map through a general affine by vote on the device (csrc/conform.hip: bts_label_resample3d, ops.label_resample3d)
against the float64 restatement tests/labelvote_ref.py: EQUAL ON EVERY VOXEL.  tests/test_labelvote_host.py ties the restatement to the
order-1 path that is pinned to SciPy and shows that these inputs hold no voxel whose decision hangs on a weight's last bit (margins >=
2e-5, no coordinate within 1e-6 of a face of the field of view), so nothing is left out; the exact ties of the two half-voxel shifts are
exact in both, and the smallest value must win them."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import conform_ref  # noqa: E402
import labelvote_ref  # noqa: E402
from conform_ref import OUT, SRC, matrices  # noqa: E402

pytestmark = pytest.mark.gpu

INT_OUT = (37, 19, 23)
_REFS = {}


def dev():
    return torch.device('cuda', 0)


def ops():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops


def reference(name):
    """volume, matrix, extent and the restatement's labels: computed once per case, left unchanged"""
    if name not in _REFS:
        y = labelvote_ref.label_volume(SRC, 21)
        if name in labelvote_ref.TIE_SHIFTS:
            m, out = labelvote_ref.shift_matrix(labelvote_ref.TIE_SHIFTS[name]), SRC
        else:
            m, out = matrices()[name], INT_OUT if name == 'integer' else OUT
        ref, margin = labelvote_ref.label_vote(y, m, out)
        ref.setflags(write=False)
        _REFS[name] = (y, m, out, ref, margin)
    return _REFS[name]


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('name', ['oblique', 'anisotropic', 'permuting', 'integer'])
def test_kernel_equals_restatement_everywhere(name, padded):
    y, m, out, ref, margin = reference(name)
    pad = tuple(s + 8 - s % 8 for s in out) if padded else out
    yg = torch.from_numpy(y).to(dev())
    got = ops().label_resample3d(yg, m, out, pad_to=pad if padded else None)
    assert tuple(got.shape) == pad + (1,) and got.dtype == torch.float32 and got.is_contiguous()
    g = got[..., 0].cpu().numpy()
    differ = g[:out[0], :out[1], :out[2]] != ref
    print('%s: %d of %d voxels differ; smallest margin of the reference %.3g' % (name, int(differ.sum()), differ.size, float(margin.min())))
    assert not differ.any()
    if padded:
        g[:out[0], :out[1], :out[2]] = 0.0
        assert not g.any()                                              # the padding
    again = ops().label_resample3d(yg.unsqueeze(-1), m, out, pad_to=pad)                  # (D,H,W,1), a second run: the same bits
    assert torch.equal(again, got)
    assert np.array_equal(yg.cpu().numpy(), y)                          # the source is left as it is


@pytest.mark.parametrize('name', sorted(labelvote_ref.TIE_SHIFTS))
def test_exact_ties_go_to_the_smallest_value(name):
    y, m, out, ref, margin = reference(name)
    tie = margin == 0.0
    assert tie.sum() >= 100
    got = ops().label_resample3d(torch.from_numpy(y).to(dev()), m, out)[..., 0].cpu().numpy()
    assert np.array_equal(got, ref)
    # said without the restatement's own tie rule: of the values whose summed weight is the largest, the smallest
    val, wt = labelvote_ref.taps(y, m, out)
    totals = np.stack([np.where(val == v, wt, 0.0).sum(axis=0) for v in labelvote_ref.VALUES])
    smallest = np.array(labelvote_ref.VALUES)[np.argmax(totals == totals.max(axis=0), axis=0)]
    assert np.array_equal(got[tie], smallest[tie].astype(np.float32))


@pytest.mark.parametrize('src,out,m', [
    ((1, 7, 5), (3, 8, 6), [[0.2871, 0.0113, 0.0057, -0.3719], [0.0531, 0.8713, 0.1037, -0.2831], [0.0173, -0.0971, 0.8117, 0.1931]]),
    ((6, 1, 5), (7, 3, 6), [[0.8713, 0.0531, 0.0113, -0.2137], [0.0057, 0.2871, 0.0173, -0.3719], [0.1037, 0.0131, 0.7919, -0.1171]]),
    ((6, 7, 1), (7, 8, 3), [[0.8713, 0.0113, 0.0531, -0.2137], [0.1037, 0.8917, 0.0131, -0.3119], [0.0057, 0.0173, 0.2871, -0.3719]]),
    ((5, 6, 7), (6, 7, 1), [[0.8513, 0.1037, 0.0, -0.3119], [0.0131, 0.8917, 0.0, -0.2137], [0.1013, 0.0531, 1.0, 2.7193]]),         # W = 1
    ((5, 6, 7), (9, 8, 11), [[1.0131, 0.1037, 0.0113, -3.6137], [0.0173, 1.1093, 0.1013, 2.3119], [0.0531, 0.0057, 0.9131, -1.7193]]),
])
def test_edges(src, out, m):
    """source extents of 1 on D, H and W, where both taps of that axis reflect onto the same voxel; an output of W = 1; and a map that
    leaves most of the output outside the field of view.  Dense random labels, so nearly every voxel sees several values"""
    rng = np.random.default_rng(5)
    y = np.array(labelvote_ref.VALUES, dtype=np.float32)[rng.integers(0, 4, size=src)]
    m = np.array(m)
    ref, margin = labelvote_ref.label_vote(y, m, out)
    fov = conform_ref.inside(m, out, src)
    assert float(margin.min()) >= 1e-9 and not conform_ref.near_a_decision(m, out, src, 1, eps=1e-6).any()
    if out == (9, 8, 11):
        assert 0.05 < fov.mean() < 0.5
    else:
        assert fov.mean() > 0.5
    got = ops().label_resample3d(torch.from_numpy(y).to(dev()), m, out)[..., 0].cpu().numpy()
    assert np.array_equal(got, ref)
    assert not got[~fov].any()


def test_any_label_values_come_through():
    values = (-3.0, 7.0, 250.0, 0.5)
    y = labelvote_ref.label_volume(SRC, 22, values)
    m = matrices()['oblique']
    ref, margin = labelvote_ref.label_vote(y, m, OUT)
    assert float(margin.min()) >= 1e-9
    got = ops().label_resample3d(torch.from_numpy(y).to(dev()), m, OUT)[..., 0].cpu().numpy()
    assert np.array_equal(got, ref)
    assert set(np.unique(got).tolist()) == set(values) | {0.0}          # 0: outside the field of view


@pytest.mark.parametrize('src,out,pad', [((9, 7, 13), (8, 9, 11), (11, 9, 12)), ((1, 2, 3), (2, 3, 1), (2, 3, 1)), ((5, 66, 4), (7, 5, 70), (7, 6, 70))])
def test_guard_bands_and_poisoned_surroundings(src, out, pad):
    """source and destination carved out of larger allocations (tests/guard_alloc.py's bands): nothing outside the destination is
    written, and the result does not depend on what surrounds either buffer"""
    import guard_alloc
    o = ops()
    rng = np.random.default_rng(9)
    yn = np.array(labelvote_ref.VALUES, dtype=np.float32)[rng.integers(0, 4, size=src)]
    lin = 0.9 * conform_ref.rotation((1.0, -2.0, 0.5), 11.0)
    m = conform_ref.about_centres(lin, src, out) + np.array([[0, 0, 0, 0.21], [0, 0, 0, -0.13], [0, 0, 0, 0.17]])
    results = []
    for fill in (guard_alloc.FILL, guard_alloc.POISON, 0x00):
        g = guard_alloc.Guarded(fill)
        y = g.empty(src, dtype=torch.float32, device=dev())
        y.copy_(torch.from_numpy(yn))
        dst = g.empty(pad + (1,), dtype=torch.float32, device=dev())
        ret = o.label_resample3d(y, m, out, pad_to=pad, out=dst)
        assert ret.data_ptr() == dst.data_ptr()
        results.append(dst.cpu().numpy().copy())
        assert g.check() == 2                                           # the bands of both buffers still hold the fill
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    ref, margin = labelvote_ref.label_vote(yn, m, out)
    assert float(margin.min()) >= 1e-9
    assert np.array_equal(results[0][:out[0], :out[1], :out[2], 0], ref)
    rest = results[0][..., 0].copy()
    rest[:out[0], :out[1], :out[2]] = 0.0
    assert not rest.any()


class Reached(Exception):
    pass


def test_bad_arguments_raise_before_the_launch(monkeypatch):
    o = ops()
    y = torch.zeros((4, 5, 6), device=dev())
    eye = np.eye(4)[:3]
    L = o.lib()
    m12 = (ctypes.c_double * 12)(*eye.reshape(-1))
    dst = torch.zeros((4, 5, 6), device=dev())

    def call(lab, ds, d, do, dp, mm):
        return L._bts_label_resample3d(lab, ds[0], ds[1], ds[2], d, do[0], do[1], do[2], dp[0], dp[1], dp[2], mm, o._stream())
    ok = (4, 5, 6)
    assert call(o._p(y), ok, o._p(dst), ok, ok, m12) == 0
    assert call(None, ok, o._p(dst), ok, ok, m12) == -1 and call(o._p(y), ok, None, ok, ok, m12) == -1
    assert call(o._p(y), ok, o._p(dst), ok, ok, None) == -1 and call(o._p(y), ok, o._p(y), ok, ok, m12) == -1
    assert call(o._p(y), (0, 5, 6), o._p(dst), ok, ok, m12) == -1 and call(o._p(y), ok, o._p(dst), (4, 0, 6), ok, m12) == -1
    assert call(o._p(y), ok, o._p(dst), ok, (4, 5, 5), m12) == -1 and call(o._p(y), ok, o._p(dst), ok, (3, 5, 6), m12) == -1
    assert call(ctypes.c_void_p(y.data_ptr() + 2), ok, o._p(dst), ok, ok, m12) == -2                 # BTS_ERR_ALIGN
    assert call(o._p(y), ok, ctypes.c_void_p(dst.data_ptr() + 1), ok, ok, m12) == -2
    torch.cuda.synchronize()
    assert not dst.any()                                                # the one good call: zeros in, zeros out; the bad ones wrote nothing

    def reached():
        raise Reached()
    monkeypatch.setattr(o._core, 'lib', reached)
    with pytest.raises(Reached):
        o.label_resample3d(y, eye, ok)
    for bad in (y.cpu(), y.double(), y[:, :, ::2], torch.zeros((4, 5, 6, 2), device=dev()), torch.zeros((5, 6), device=dev()),
                torch.zeros((4, 5, 6), dtype=torch.uint8, device=dev())):
        with pytest.raises(ValueError):
            o.label_resample3d(bad, eye, ok)
    for kw in (dict(matrix=np.eye(3)), dict(out_shape=(4, 0, 6)), dict(pad_to=(4, 4, 6)), dict(out=torch.zeros((4, 5, 6), device=dev())),
               dict(out=torch.zeros((4, 5, 6, 1), dtype=torch.float64, device=dev())), dict(out=y.view(4, 5, 6, 1))):
        args = dict(matrix=eye, out_shape=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            o.label_resample3d(y, **args)
