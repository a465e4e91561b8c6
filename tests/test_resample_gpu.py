"""-m gpu: device-side spline resampling (csrc/resample.hip: bts_spline_prefilter3d, bts_zoom3d) and the Interpolator / segment_scan
wrappers against scipy.ndimage.zoom per channel.

The GPU box may have no SciPy: the oracle is tests/golden/resample_vectors.npz (SciPy in float64, written by make_resample_golden.py)
and, at sizes too large to commit, the float64 restatement tests/zoom_ref.py, whose equality with SciPy tests/test_resample_host.py
proves.  Tolerances are never taken from the kernel under test:

  order 3   per case 4 x the float32 restatement's own max deviation from the float64 reference, computed here on the CPU (the factor
            covers another summation order of the 64 taps and FMA contraction); the observed kernel / restatement ratio is printed
  order 1   2 ulp of max|ref| (float32 spacing at that magnitude);  order 0   bit-equal
  mask      a voxel may differ from the reference mask only where |max_c reference| <= the case's tolerance, on at most 0.1 % of voxels
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import zoom_ref  # noqa: E402

pytestmark = pytest.mark.gpu

from oracle import torch_ref as R  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'resample_vectors.npz'))
SPEC = json.loads(str(GOLDEN['spec']))
NAMES = [c['name'] for c in SPEC]


def dev():
    return torch.device('cuda', 0)


def case_of(name):
    c = [c for c in SPEC if c['name'] == name][0]
    x = GOLDEN[name + '_x']
    shape = tuple(c['out_shape']) if 'out_shape' in c else zoom_ref.zoom_output_shape(x.shape[:3], c['factors'])
    return c, x, GOLDEN[name + '_y'].astype(np.float64), shape


def max_dev(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max())


def check_mask(mask, ref, tol, what):
    """the pointwise mask criterion of the module docstring"""
    ref_max = ref.max(axis=-1)
    differ = (np.asarray(mask)[..., 0] > 0) != (ref_max > 0)
    outside = differ & (np.abs(ref_max) > tol)
    print('%s: mask differs on %d of %d voxels (%.4f %%), %d of them where |max_c ref| > tol %.3g'
          % (what, int(differ.sum()), differ.size, 100.0 * differ.mean(), int(outside.sum()), tol))
    assert int(outside.sum()) == 0, what
    assert differ.mean() <= 1e-3, what
    assert set(np.unique(np.asarray(mask)).tolist()) <= {0.0, 1.0}


def gpu_zoom(x, shape, order, **kw):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    xg = torch.from_numpy(x).to(dev())
    coef = ops.spline_prefilter3d(xg) if order == 3 else xg
    return ops.zoom3d(coef, shape, order=order, **kw)


@pytest.mark.parametrize('name', NAMES)
def test_prefilter_matches_restatement(name):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    _, x, _, _ = case_of(name)
    ref = zoom_ref.prefilter3d(x, np.float64)
    tol = 4.0 * max_dev(zoom_ref.prefilter3d(x, np.float32), ref)
    xg = torch.from_numpy(x).to(dev())
    out = ops.spline_prefilter3d(xg)
    err = max_dev(out.cpu().numpy(), ref)
    print('%s prefilter: kernel max dev %.3g, float32 restatement %.3g, ratio %.2f' % (name, err, tol / 4, err / (tol / 4)))
    assert err <= tol
    again = ops.spline_prefilter3d(xg.clone(), out=torch.empty_like(xg))
    assert torch.equal(out, again)
    inplace = xg.clone()
    ops.spline_prefilter3d(inplace, out=inplace)               # src == dst is part of the ABI
    assert torch.equal(out, inplace)


@pytest.mark.parametrize('name', NAMES)
def test_zoom_chain_matches_scipy_golden(name):
    c, x, ref, shape = case_of(name)
    order = c['order']
    y, mask = gpu_zoom(x, shape, order, want_mask=True)
    torch.cuda.synchronize()
    assert tuple(y.shape) == shape + (x.shape[-1],) and tuple(mask.shape) == shape + (1,)
    yc = y.cpu().numpy()
    scale = float(np.abs(ref).max())
    if order == 0:
        assert np.array_equal(yc, ref.astype(np.float32)), name
        tol = 0.0
    elif order == 1:
        tol = 2.0 * float(np.spacing(np.float32(scale)))
        err = max_dev(yc, ref)
        print('%s: order 1 kernel max dev %.3g = %.2f ulp of max|ref|' % (name, err, err / (tol / 2)))
        assert err <= tol
    else:
        r32 = max_dev(zoom_ref.zoom(x, shape, 3, np.float32), ref)
        tol = 4.0 * r32
        err = max_dev(yc, ref)
        print('%s: kernel max dev %.3g (%.2g of max|ref|), float32 restatement %.3g, ratio %.2f' % (name, err, err / scale, r32, err / r32))
        assert err <= tol
    check_mask(mask.cpu().numpy(), ref, tol, name)
    y2, mask2 = gpu_zoom(x, shape, order, want_mask=True)      # bitwise determinism over two runs
    assert torch.equal(y, y2) and torch.equal(mask, mask2)


def test_padding_is_zero_and_equals_pad_to_spatial_res():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c, x, ref, shape = case_of('cubic_c4_padmask')
    res = c['pad_res']
    it = infer.Interpolator(None, order=3)
    y, m = it.resample(x, c['factors'])
    yp, mp, orig = it.resample(torch.from_numpy(x).to(dev()), c['factors'], pad_res=res)
    assert list(orig) == list(shape) and tuple(y.shape[:3]) == shape
    padded = tuple(s + res - s % res for s in shape)
    assert tuple(yp.shape) == padded + (4,) and tuple(mp.shape) == padded + (1,)
    outside = torch.ones(padded, dtype=torch.bool, device=dev())
    outside[:shape[0], :shape[1], :shape[2]] = False
    assert float(yp[outside].abs().max()) == 0.0 and float(mp[outside].abs().max()) == 0.0
    xr, mr, origr = infer.pad_to_spatial_res(res, y, m)
    assert torch.equal(xr, yp) and torch.equal(mr, mp) and list(origr) == list(orig)
    tol = 4.0 * max_dev(zoom_ref.zoom(x, shape, 3, np.float32), ref)
    assert max_dev(y.cpu().numpy(), ref) <= tol
    check_mask(m.cpu().numpy(), ref, tol, 'resample(pad_res=None)')
    # mean / std are applied after the mask test, to the padding as well: the result is the normalised padded volume
    from bts_amd import ops
    mean = torch.tensor([95.0, 110.0, 80.0, 120.0], device=dev())
    std = torch.tensor([35.0, 45.0, 25.0, 50.0], device=dev())
    coef = ops.spline_prefilter3d(torch.from_numpy(x).to(dev()))
    yn, mn = ops.zoom3d(coef, shape, pad_to=padded, want_mask=True, mean=mean, std=std)
    assert torch.equal(mn, mp)
    assert float((yn - (yp - mean) / std).abs().max()) <= 1e-5


def test_unit_pixdim_skips_the_resample():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    _, x, _, _ = case_of('cubic_c2_mixed')
    it = infer.Interpolator(None)
    y, m = it.resample(x, (1.0, 1.0, 1.0))
    assert np.array_equal(y.cpu().numpy(), x)
    assert np.array_equal(m.cpu().numpy(), zoom_ref.brain_mask(x))


def test_reverse_to_an_explicit_native_shape():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c, x, ref, shape = case_of('cubic_c1_reverse')
    it = infer.Interpolator(None, order=3)
    native = np.zeros(shape + (1,), np.float32)
    y1, m1 = it.resample(native, (1.3, 0.9, 0.8))
    assert tuple(y1.shape[:3]) == x.shape[:3]                  # the 1 mm^3 grid of that scan is the golden case's input grid
    p = torch.from_numpy(x / np.float32(x.max())).to(dev())
    bm = torch.from_numpy(zoom_ref.brain_mask(x)).to(dev())
    y, lab = it.reverse(p, mask=bm)
    assert tuple(y.shape) == shape + (1,) and tuple(lab.shape) == shape and lab.dtype == torch.uint8
    pref = zoom_ref.zoom(x / np.float32(x.max()), shape, 3, np.float64)
    mref = zoom_ref.zoom(zoom_ref.brain_mask(x), shape, 0, np.float64)
    tol = 4.0 * max_dev(zoom_ref.zoom(x / np.float32(x.max()), shape, 3, np.float32), pref)
    assert max_dev(y.cpu().numpy(), pref * mref) <= tol
    lab_ref = R.tta_labels(torch.from_numpy(pref * mref), torch.from_numpy(mref), 0.5)
    differ = (lab.cpu() != lab_ref).numpy()
    assert not np.any(differ & (np.abs(pref[..., 0] * mref[..., 0] - 0.5) > 2 * tol))


def full_size_input():
    """155x190x147x4 scan-like volume: smooth tissue up to ~1000 per modality around an exactly-zero cavity"""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in (155, 190, 147)], indexing='ij')
    tex = 0.65 + 0.35 * np.sin(9.0 * g[0] + 1.0) * np.cos(7.0 * g[1] + 2.0) * np.sin(11.0 * g[2] + 0.5)
    chans = []
    for c, a in enumerate((950.0, 700.0, 480.0, 820.0)):
        r2 = ((g[0] - 0.02 * c) / 0.3) ** 2 + (g[1] / 0.25) ** 2 + ((g[2] + 0.02 * c) / 0.3) ** 2
        chans.append(np.where(r2 < 1.0, 0.0, tex * a))
    return np.stack(chans, axis=-1).astype(np.float32)


def test_full_size_scan_matches_float64_restatement():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    x = full_size_input()
    shape = infer.zoom_output_shape(x.shape[:3], (1.2, 0.9, 1.5))
    assert shape == (186, 171, 220)
    it = infer.Interpolator(None, order=3)
    y, m = it.resample(x, (1.2, 0.9, 1.5))
    torch.cuda.synchronize()
    ref = zoom_ref.zoom(x, shape, 3, np.float64)
    r32 = max_dev(zoom_ref.zoom(x, shape, 3, np.float32), ref)
    err = max_dev(y.cpu().numpy(), ref)
    print('full size: kernel max dev %.3g (%.2g of max|ref|), float32 restatement %.3g, ratio %.2f'
          % (err, err / np.abs(ref).max(), r32, err / r32))
    assert err <= 4.0 * r32
    check_mask(m.cpu().numpy(), ref, 4.0 * r32, 'full size')
    y2, m2 = it.resample(x, (1.2, 0.9, 1.5))
    assert torch.equal(y, y2) and torch.equal(m, m2)


def test_offsets_past_two_gigabytes():
    """a destination of 2.2e9 bytes: voxel offsets times C pass 2^31 and byte offsets 2^32 / 2; order 0 is a pure gather, so torch's
    own indexing is the reference"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn((40, 50, 30, 4), generator=g).to(dev())
    shape = (800, 820, 210)
    y, m = ops.zoom3d(x, shape, order=0, want_mask=True)
    assert y.numel() * 4 > 2 ** 31
    idx = [torch.from_numpy(zoom_ref.taps(n, o, 0, np.float32)[0][:, 0]).to(dev()) for n, o in zip(x.shape[:3], shape)]
    for d0 in (0, 400, 790):                                   # slabs of 10 planes: first, middle, last
        sl = slice(d0, d0 + 10)
        ref = x[idx[0][sl]][:, idx[1]][:, :, idx[2]]
        assert torch.equal(y[sl], ref)
        assert torch.equal(m[sl, ..., 0], (ref.max(dim=-1).values > 0).float())


@pytest.mark.parametrize('C,order,vol,out,pad', [(3, 3, (9, 7, 13), (11, 5, 29), (16, 8, 32)), (1, 3, (5, 66, 4), (7, 40, 9), (7, 40, 9)),
                                                 (8, 1, (4, 5, 6), (9, 3, 6), (10, 3, 7)), (5, 0, (1, 2, 3), (4, 4, 4), (5, 4, 4)),
                                                 (2, 3, (4, 5, 4200), (3, 4, 17), (3, 4, 17))])
def test_guard_bands_around_dst_and_mask(C, order, vol, out, pad):
    """4 KB of 0xA5 on either side of coef, dst and mask, carved out of larger allocations: ragged row tiles, odd channel counts, a
    W row too wide for the LDS tile, extents of 1, padding on some axes only"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    PAD, FILL = 4096, 0xA5
    live = []

    def guarded(shape):
        n = int(np.prod(shape)) * 4
        big = torch.full((n + 2 * PAD,), FILL, dtype=torch.uint8, device=dev())
        live.append((big, n))
        return big[PAD:PAD + n].view(torch.float32).view(shape)

    g = torch.Generator().manual_seed(11)
    x = torch.randn(vol + (C,), generator=g).to(dev())
    coef = guarded(vol + (C,))
    if order == 3:
        ops.spline_prefilter3d(x, out=coef)
        ref = zoom_ref.prefilter3d(x.cpu().numpy(), np.float32)
        assert np.abs(coef.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
    else:
        coef.copy_(x)
    dst, mask = guarded(pad + (C,)), guarded(pad + (1,))
    ops.lib().call('bts_zoom3d', ops._p(coef), ops._p(dst), ops._p(mask), None, None, vol[0], vol[1], vol[2], out[0], out[1], out[2], C,
                   pad[0], pad[1], pad[2], order, ops._stream())
    torch.cuda.synchronize()
    for big, n in live:
        assert bool((big[:PAD] == FILL).all()) and bool((big[PAD + n:] == FILL).all()), 'a guard band was written'
    ref = zoom_ref.interpolate(coef.cpu().numpy(), out, order, np.float32)
    got = dst[:out[0], :out[1], :out[2]].cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    inside = torch.zeros(pad, dtype=torch.bool, device=dev())
    inside[:out[0], :out[1], :out[2]] = True
    if not bool(inside.all()):
        assert float(dst[~inside].abs().max()) == 0.0 and float(mask[~inside].abs().max()) == 0.0


def test_bad_arguments_are_refused():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x = torch.zeros((8, 8, 8, 2), device=dev())
    with pytest.raises(ValueError):
        ops.spline_prefilter3d(x[..., :1])                     # not dense
    with pytest.raises(ValueError):
        ops.zoom3d(x[0], (4, 4, 4))                            # wrong rank
    with pytest.raises(ValueError):
        ops.zoom3d(x, (4, 4, 4), order=2)
    with pytest.raises(ValueError):
        ops.zoom3d(x, (4, 4, 4), pad_to=(4, 3, 4))
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.spline_prefilter3d(torch.zeros((3, 8, 8, 2), device=dev()))
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.spline_prefilter3d(torch.zeros((8, 8, 8, 9), device=dev()))


def randomised_params(cfg, crop, seed):
    P = R.build_params(cfg, crop, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in P:
        if k.endswith('_b'):
            P[k] = torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.1
        if k.endswith('_g'):
            P[k] = 1.0 + torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.3
    for k in P:
        P[k] = P[k].float().double()
    return P


def small_model(kw, padded):
    from bts_amd.model import Model
    cfg = R.default_config(**kw)
    P = randomised_params(cfg, tuple(padded), seed=5)
    m = Model(**kw)
    m.build((1,) + tuple(padded) + (2,))
    m.set_weights_from(P)
    return m


def scan_like(vol, seed):
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in vol], indexing='ij')
    rng = np.random.default_rng(seed)
    tex = 0.65 + 0.35 * np.sin(5.0 * g[0] + 1.0) * np.cos(4.0 * g[1] + 2.0) * np.sin(6.0 * g[2] + 0.5) + 0.02 * rng.standard_normal(vol)
    chans = []
    for c, a in enumerate((160.0, 190.0)):
        r2 = ((g[0] - 0.05 * c) / 0.3) ** 2 + (g[1] / 0.25) ** 2 + (g[2] / 0.35) ** 2
        chans.append(np.where(r2 < 1.0, 0.0, tex * a))
    return np.stack(chans, axis=-1).astype(np.float32)


def test_segment_scan_with_unit_pixdim_is_segment_volume():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    kw, vol, res = dict(base_filters=8, groups=2, reduction=2, depth=3), (13, 9, 16), 8
    x = torch.from_numpy(scan_like(vol, 4)).to(dev())
    mask = (x.max(dim=-1, keepdim=True).values > 0).float()
    assert 0.0 < float(mask.mean()) < 1.0
    mean, std = torch.tensor([95.0, 110.0]), torch.tensor([35.0, 45.0])
    m = small_model(kw, tuple(s + res - s % res for s in vol))
    y0, lab0 = infer.segment_volume(m, x, mask, mean, std, res)
    y1, lab1 = infer.segment_scan(m, x, (1.0, 1.0, 1.0), mean, std, res)
    assert torch.equal(y0, y1) and torch.equal(lab0, lab1)
    y2, lab2 = infer.segment_scan(m, x.cpu().numpy(), (1, 1, 1), mean, std, res, tta_batch=1)
    assert torch.equal(y0, y2) and torch.equal(lab0, lab2)


def test_segment_scan_matches_the_restated_chain():
    """40x48x32x2 scan with pixdim (1.2, 0.9, 1.5): native-grid probabilities against
         float64-restatement resample -> product segment_volume -> float64-restatement reverse.
    Bound, derived here and not guessed: the product's 1 mm^3 input may differ from the restated one by the resample tolerance (4 x the
    float32 restatement's deviation e32 from float64).  That tolerance is pushed through the network by a second forward on the input
    perturbed by 4 * e32 voxel for voxel; the largest probability change dP is what the tolerance becomes at the network's output.
    The way back is linear: per axis the cubic prefilter is the convolution with h[k] = sqrt(3) z^|k|, z = sqrt(3) - 2, whose absolute
    sum is sqrt(3) (1+|z|)/(1-|z|) = 3, so it amplifies a bounded error by at most 3^3 = 27; the B-spline weights are positive and sum
    to 1; the mask is 0 or 1; and the reverse has its own 4 x float32-restatement tolerance.  So |dp_native| <= 27 dP + tol_reverse.
    The input keeps |max_c| of the restated 1 mm^3 volume above the resample tolerance everywhere, so the mask criterion leaves the
    product's mask no voxel to differ on (asserted below as a precondition on the input, not on the kernel).  Labels: the pointwise
    criterion of tests/test_oracle_fullsize_gpu.py (a label may differ only where the reference margin <= 2 |dp| at that voxel)."""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    kw, vol, res, pixdim = dict(base_filters=8, groups=2, reduction=2, depth=3), (40, 48, 32), 8, (1.2, 0.9, 1.5)
    x = scan_like(vol, 9)
    shape = infer.zoom_output_shape(vol, pixdim)
    assert shape == (48, 43, 48)
    mean, std = torch.tensor([95.0, 110.0]), torch.tensor([35.0, 45.0])
    m = small_model(kw, tuple(s + res - s % res for s in shape))
    y, lab = infer.segment_scan(m, x, pixdim, mean, std, res)
    torch.cuda.synchronize()
    assert tuple(y.shape) == vol + (3,) and tuple(lab.shape) == vol and lab.dtype == torch.uint8

    r64 = zoom_ref.zoom(x, shape, 3, np.float64)
    r32 = zoom_ref.zoom(x, shape, 3, np.float32)
    mref = zoom_ref.brain_mask(r64)
    e32 = max_dev(r32, r64)
    assert float(np.abs(r64.max(axis=-1)).min()) > 4.0 * e32   # precondition: no voxel sits within the resample tolerance of the mask cut
    assert np.array_equal(mref, zoom_ref.brain_mask(r32)) and 0.0 < mref.mean() < 1.0
    x1 = torch.from_numpy(r64.astype(np.float32)).to(dev())
    x1p = torch.from_numpy((r64 + 4.0 * (r32.astype(np.float64) - r64)).astype(np.float32)).to(dev())
    mg = torch.from_numpy(mref).to(dev())
    p_ref, _ = infer.segment_volume(m, x1, mg, mean, std, res)
    p_pert, _ = infer.segment_volume(m, x1p, mg, mean, std, res)
    dP = float((p_pert - p_ref).abs().max())
    p_ref = p_ref.cpu().numpy()
    back = zoom_ref.zoom(p_ref, vol, 3, np.float64)
    tol_rev = 4.0 * max_dev(zoom_ref.zoom(p_ref, vol, 3, np.float32), back)
    mback = zoom_ref.zoom(mref, vol, 0, np.float64)
    ref = back * mback
    bound = 27.0 * dP + tol_rev
    d = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    print('segment_scan vs restated chain: max |dp| %.3g; bound %.3g = 27 * dP %.3g + reverse tol %.3g' % (d.max(), bound, dP, tol_rev))
    assert dP > 0.0
    assert d.max() <= bound
    lab_ref = R.tta_labels(torch.from_numpy(ref), torch.from_numpy(mback), 0.5)
    top2 = np.sort(ref, axis=-1)[..., ::-1][..., :2]
    margin = np.minimum(np.abs(top2[..., 0] - 0.5), np.abs(top2[..., 0] - top2[..., 1]))
    differ = (lab.cpu() != lab_ref).numpy()
    outside = differ & (margin > 2.0 * d.max(axis=-1))
    print('labels: %d of %d differ, %d outside the pointwise criterion' % (int(differ.sum()), differ.size, int(outside.sum())))
    assert int(outside.sum()) == 0
    assert set(np.unique(lab.cpu().numpy()).tolist()) <= {0, 1, 2, 4}
