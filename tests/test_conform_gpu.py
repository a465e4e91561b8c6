"""-m gpu: conforming a scan to an oriented grid by its affine on the device (csrc/conform.hip: bts_reorient3d, bts_affine_resample3d; the
infer.Conformer and segment_case(geometry=...) above them) against the float64 restatement tests/conform_ref.py, whose equality with
scipy.ndimage.affine_transform tests/test_conform_host.py proves.  Extents are odd and unequal, so tiles and rows end mid-way and no two
axes can be confused.  Tolerances are those of tests/test_resample_gpu.py and never taken from the kernel under test:

  reorientation   bit-equal to numpy
  order 0         bit-equal;   order 1   2 ulp of max|ref| (float32 spacing at that magnitude)
  order 3         4 x the float32 restatement's own max deviation from the float64 one, computed here; the observed ratio is printed
  left out        voxels whose float64 coordinate lies within 1e-6 of a face of the field of view or of an order-0 rounding tie, where the
                  coordinate's last bit decides; at most 0.1 % of the voxels, and none for an integer map
  mask            a voxel may differ from the reference mask only where |max_c reference| <= the case's tolerance, on at most 0.1 %
"""
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
import zoom_ref  # noqa: E402
from conform_ref import OUT, SRC, matrices, volume  # noqa: E402

pytestmark = pytest.mark.gpu

from oracle import torch_ref as R  # noqa: E402

PERMS = sorted({conform_ref.reorientation(code, 'LPS') for code in conform_ref.all_codes()})
LPS = np.array([[-1.0, 0, 0, 90], [0, -1, 0, 126], [0, 0, 1, -72], [0, 0, 0, 1]])


def dev():
    return torch.device('cuda', 0)


def max_dev(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max())


def check_mask(mask, ref, tol, what):
    """the pointwise mask criterion of the module docstring (tests/test_resample_gpu.py)"""
    ref_max = ref.max(axis=-1)
    differ = (np.asarray(mask)[..., 0] > 0) != (ref_max > 0)
    outside = differ & (np.abs(ref_max) > tol)
    print('%s: mask differs on %d of %d voxels, %d of them where |max_c ref| > tol %.3g' % (what, int(differ.sum()), differ.size,
                                                                                          int(outside.sum()), tol))
    assert int(outside.sum()) == 0, what
    assert differ.mean() <= 1e-3, what
    assert set(np.unique(np.asarray(mask)).tolist()) <= {0.0, 1.0}


# ---- bts_reorient3d ----
@pytest.mark.parametrize('C,shape', [(1, (19, 23, 37)), (2, (19, 23, 37)), (4, (19, 23, 37)),       # W * C = 37, 74, 148: no multiple of 64
                                     (2, (70, 1, 67)), (1, (66, 5, 130)), (3, (5, 66, 9)), (8, (9, 35, 11))])
def test_reorient_all_signed_permutations_bit_equal(C, shape):
    """48 signed permutations per case; the extra shapes have an axis of length 1, more than one tile along either tiled axis for their
    channel count (TI = 64 / C voxels by 64 or 32 lines) and channel counts that do not divide the tile"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    assert len(PERMS) == 48
    g = torch.Generator().manual_seed(7)
    x = torch.randn(shape + (C,), generator=g)
    xn, xg = x.numpy(), x.to(dev())
    for perm, flip in PERMS:
        want = np.flip(np.transpose(xn, perm + (3,)), [a for a in range(3) if flip[a]])
        got = ops.reorient3d(xg, perm, flip)
        assert tuple(got.shape) == want.shape and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), want), (perm, flip)
    assert np.array_equal(xg.cpu().numpy(), xn)                                       # the source is left as it is


def test_reorient_refuses_bad_arguments():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x = torch.zeros((4, 5, 6, 2), device=dev())
    with pytest.raises(ValueError):
        ops.reorient3d(x, (0, 1, 1), (False, False, False))
    with pytest.raises(ValueError):
        ops.reorient3d(x, (0, 1, 2), (False, False))
    with pytest.raises(ValueError):
        ops.reorient3d(x[..., :1], (0, 1, 2), (False, False, False))                  # not dense
    with pytest.raises(ValueError):
        ops.reorient3d(x, (0, 1, 2), (True, False, False), out=x)                     # in place
    with pytest.raises(ValueError):
        ops.reorient3d(x, (1, 0, 2), (False, False, False), out=torch.empty_like(x))  # the shape of the transposed volume
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.reorient3d(torch.zeros((4, 5, 6, 9), device=dev()), (0, 1, 2), (False, False, False))
    with pytest.raises(ValueError):
        ops.affine_resample3d(x, np.eye(4)[:3], (4, 5, 6), order=2)
    with pytest.raises(ValueError):
        ops.affine_resample3d(x, np.eye(3), (4, 5, 6))
    with pytest.raises(ValueError):
        ops.affine_resample3d(x, np.eye(4)[:3], (4, 5, 6), pad_to=(4, 4, 6))
    with pytest.raises(ValueError):
        ops.affine_resample3d(x, np.eye(4)[:3], (4, 5, 6), channel=1)                 # no volume to write into
    wide = torch.zeros((4, 5, 6, 4), device=dev())
    with pytest.raises(ValueError):
        ops.affine_resample3d(x, np.eye(4)[:3], (4, 5, 6), out=wide, channel=3)       # channels 3, 4 of 4
    with pytest.raises(ValueError):
        ops.affine_resample3d(x, np.eye(4)[:3], (4, 5, 6), out=wide, channel=0, want_mask=True)


# ---- bts_affine_resample3d ----
_REFS = {}


def reference(name, order, C):
    """float64 restatement, float32 restatement's deviation from it, the voxels left out: computed once per case"""
    key = (name, order, C)
    if key not in _REFS:
        m = matrices()[name]
        out = (37, 19, 23) if name == 'integer' else OUT
        x = volume(SRC, C, 11)
        ref = conform_ref.affine_resample(x, m, out, order, np.float64)
        r32 = max_dev(conform_ref.affine_resample(x, m, out, order, np.float32), ref) if order == 3 else 0.0
        near = conform_ref.near_a_decision(m, out, SRC, order, eps=1e-6)
        if name == 'integer':
            assert not near.any()                                                     # checked on every voxel
        assert near.mean() <= 1e-3
        ref.setflags(write=False)
        _REFS[key] = (m, out, x, ref, r32, near)
    return _REFS[key]


@pytest.mark.parametrize('C', [1, 4])
@pytest.mark.parametrize('order', [0, 1, 3])
@pytest.mark.parametrize('name', ['oblique', 'anisotropic', 'permuting', 'integer'])
def test_affine_resample_matches_float64_restatement(name, order, C):
    """C == 1 is written into channel 1 of a 4-channel volume whose other channels must come back bit-unchanged; C == 4 fills the volume
    and gives the mask.  Both with padding on every axis."""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    m, out, x, ref, r32, near = reference(name, order, C)
    pad = tuple(s + 8 - s % 8 for s in out)
    xg = torch.from_numpy(x).to(dev())
    coef = ops.spline_prefilter3d(xg) if order == 3 else xg
    g = torch.Generator().manual_seed(3)
    before = torch.randn(pad + (4,), generator=g).to(dev())
    dst = before.clone()
    if C == 1:
        ret = ops.affine_resample3d(coef, m, out, order=order, pad_to=pad, out=dst, channel=1)
        assert ret.data_ptr() == dst.data_ptr()
        assert torch.equal(dst[..., 0], before[..., 0]) and torch.equal(dst[..., 2:], before[..., 2:])
        got, mask = dst[..., 1:2], None
    else:
        got, mask = ops.affine_resample3d(coef, m, out, order=order, pad_to=pad, out=dst, channel=0, want_mask=True)
    torch.cuda.synchronize()
    inside = torch.zeros(pad, dtype=torch.bool, device=dev())
    inside[:out[0], :out[1], :out[2]] = True
    assert float(got[~inside].abs().max()) == 0.0                                     # the padding
    y = got[:out[0], :out[1], :out[2]].cpu().numpy()
    fov = conform_ref.inside(m, out, SRC)
    assert float(np.abs(y[~fov & ~near]).max(initial=0.0)) == 0.0                     # outside the field of view
    keep = ~near
    scale = float(np.abs(ref).max())
    if order == 0:
        tol = 0.0
        assert np.array_equal(y[keep], ref[keep].astype(np.float32)), name
    elif order == 1:
        tol = 2.0 * float(np.spacing(np.float32(scale)))
        err = max_dev(y[keep], ref[keep])
        print('%s C=%d: order 1 kernel max dev %.3g = %.2f ulp of max|ref|' % (name, C, err, err / (tol / 2)))
        assert err <= tol
    else:
        tol = 4.0 * r32
        err = max_dev(y[keep], ref[keep])
        print('%s C=%d: kernel max dev %.3g (%.2g of max|ref|), float32 restatement %.3g, ratio %.2f' % (name, C, err, err / scale, r32, err / r32))
        assert err <= tol
    if mask is not None:
        assert float(mask[~inside].abs().max()) == 0.0
        mk = mask[:out[0], :out[1], :out[2]].cpu().numpy()
        ref_k = np.where(near[..., None], y.astype(np.float64), ref)                  # a left-out voxel: the mask of the value it got
        check_mask(mk, ref_k, tol, '%s order %d' % (name, order))
        again, mask2 = ops.affine_resample3d(coef, m, out, order=order, pad_to=pad, want_mask=True)     # a volume of its own: same bits
        assert torch.equal(again, got) and torch.equal(mask2, mask)


@pytest.mark.parametrize('C', [1, 2, 4])
def test_integer_signed_permutation_is_the_reorientation(C):
    """an integer signed permutation gives, at orders 0 and 1, the bits of bts_reorient3d"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(SRC + (C,), generator=g).to(dev())
    for perm, flip in PERMS[::5] + [((2, 0, 1), (False, True, False))]:
        m = np.zeros((3, 4))
        for a in range(3):
            m[perm[a], a] = -1.0 if flip[a] else 1.0
            m[perm[a], 3] = SRC[perm[a]] - 1 if flip[a] else 0.0
        want = ops.reorient3d(x, perm, flip)
        for order in (0, 1):
            got = ops.affine_resample3d(x, m, tuple(want.shape[:3]), order=order)
            assert torch.equal(got, want), (perm, flip, order)


# ---- Conformer ----
def label_like(shape, seed):
    """a probability-like volume: smooth blobs in [0, 1] on an exactly-zero background"""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    rng = np.random.default_rng(seed)
    out = []
    for c in range(2):
        cx = rng.uniform(-0.3, 0.3, 3)
        r2 = sum(((g[k] - cx[k]) / (0.45 + 0.1 * c)) ** 2 for k in range(3))
        out.append(np.where(r2 < 1.0, 0.2 + 0.8 * np.cos(0.5 * np.pi * r2) ** 2, 0.0))
    return [v.astype(np.float32) for v in out]


def through_nifti(tmp_path, name, array, affine):
    """write and read back: (array, best affine)"""
    import bts_amd  # noqa: F401
    from bts_amd import nifti
    path = str(tmp_path / (name + '.nii.gz'))
    nifti.save(path, array, affine)
    data, header = nifti.load(path)
    return np.asarray(data), nifti.best_affine(header)


def ras_copy(array, affine):
    """the same scan stored with the first two array axes reversed"""
    v = np.eye(4)
    v[0, 0], v[0, 3], v[1, 1], v[1, 3] = -1.0, array.shape[0] - 1, -1.0, array.shape[1] - 1
    return np.ascontiguousarray(array[::-1, ::-1]), affine @ v


def test_conformer_ras_round_trip_is_exact(tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    lps = label_like(SRC, 1)
    vols, affs = [], []
    for c, v in enumerate(lps):
        arr, aff = through_nifti(tmp_path, 'ras%d' % c, *ras_copy(v, LPS))
        vols.append(arr)
        affs.append(aff)
    conf = infer.Conformer('LPS')
    x, m, orig = conf.forward(vols, affs)
    assert list(orig) == list(SRC) and conf.last['code'] == 'RAS' and conf.last['reorient'] == [((0, 1, 2), (True, True, False))]
    want = np.stack(lps, -1)
    assert np.array_equal(x.cpu().numpy(), want)                                      # the LPS array, bit for bit
    assert np.array_equal(m.cpu().numpy(), zoom_ref.brain_mask(want))
    xp, mp, orig = conf.forward(vols, affs, pad_res=8)
    xr, mr, _ = infer.pad_to_spatial_res(8, x, m)
    assert torch.equal(xp, xr) and torch.equal(mp, mr)
    y, lab = conf.reverse(x, path=str(tmp_path))
    assert np.array_equal(y.cpu().numpy(), np.stack(vols, -1))                        # and back: the RAS array, bit for bit
    lab_lps = R.tta_labels(torch.from_numpy(want.astype(np.float64)), torch.from_numpy(zoom_ref.brain_mask(want).astype(np.float64)), 0.5)
    assert np.array_equal(lab.cpu().numpy(), lab_lps.numpy()[::-1, ::-1])
    from bts_amd import nifti
    data, header = nifti.load(str(tmp_path / 'mask.nii'))
    assert np.array_equal(np.asarray(data), lab.cpu().numpy()) and np.allclose(header['affine'], affs[0])


def test_conformer_asl_two_millimetre_scan_matches_restatement(tmp_path):
    """an 'ASL' scan with 1 x 1 x 2 mm voxels: resampled onto the LPS 1 mm grid and back, against the restatement's plan and arithmetic"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    asl = np.eye(4)
    asl[:3, :3] = conform_ref.signed_permutation_affine('ASL', (1.0, 1.0, 2.0))
    asl[:3, 3] = (40.0, -60.0, 12.0)
    vols, affs = [], []
    for c, v in enumerate(label_like(SRC, 2)):
        arr, aff = through_nifti(tmp_path, 'asl%d' % c, v, asl)
        vols.append(arr)
        affs.append(aff)
    conf = infer.Conformer('LPS', order=3)
    x, m, orig = conf.forward(vols, affs)
    shape, target, mats = conform_ref.plan([SRC, SRC], affs)
    assert shape == (74, 19, 23) == tuple(orig) and conf.last['code'] == 'ASL' and conf.last['reorient'] == [None]
    src = np.stack(vols, -1)
    ref = conform_ref.affine_resample(src, mats[0], shape, 3, np.float64)
    assert not conform_ref.near_a_decision(mats[0], shape, SRC, 3).any() and conform_ref.inside(mats[0], shape, SRC).all()
    r32 = max_dev(conform_ref.affine_resample(src, mats[0], shape, 3, np.float32), ref)
    err = max_dev(x.cpu().numpy(), ref)
    print('ASL forward: kernel max dev %.3g, float32 restatement %.3g, ratio %.2f' % (err, r32, err / r32))
    assert err <= 4.0 * r32
    # the zero background rings at +-1e-30 after the prefilter, so the reference mask says nothing there; the mask is that of the values
    assert np.array_equal(m.cpu().numpy(), zoom_ref.brain_mask(x.cpu().numpy()))
    # back: the probabilities at order 3 through the inverse map
    p = x.cpu().numpy()
    inv = np.linalg.inv(np.concatenate([mats[0], [[0, 0, 0, 1.0]]]))[:3]
    # with an all-ones mask: at 2 : 1 every native voxel centre lies exactly between two target voxels, a rounding tie of the order-0 mask
    y, lab = conf.reverse(x, mask=torch.ones_like(m))
    assert tuple(y.shape) == SRC + (2,) and tuple(lab.shape) == SRC and lab.dtype == torch.uint8
    assert conform_ref.inside(inv, SRC, shape).all() and not conform_ref.near_a_decision(inv, SRC, shape, 3).any()
    back = conform_ref.affine_resample(p, inv, SRC, 3, np.float64)
    b32 = max_dev(conform_ref.affine_resample(p, inv, SRC, 3, np.float32), back)
    err = max_dev(y.cpu().numpy(), back)
    print('ASL reverse: kernel max dev %.3g, float32 restatement %.3g, ratio %.2f' % (err, b32, err / b32))
    assert err <= 4.0 * b32


def test_conformer_places_modalities_on_shifted_grids():
    """the second modality lies on a grid of its own -- another extent, 0.9 mm voxels, shifted by 2.5 mm -- and lands where the
    restatement puts it; the first, already LPS 1 mm, is copied; the third shares the first one's grid but not its launch"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    a, _ = label_like(SRC, 3)
    b, _ = label_like((21, 25, 33), 4)
    c, _ = label_like(SRC, 5)
    other = LPS.copy()
    other[:3, :3] *= 0.9
    other[0, 3] += 2.5
    conf = infer.Conformer('LPS', order=3)
    x, m, orig = conf.forward([a, b, c], [LPS, other, LPS], pad_res=8)
    assert conf.last['groups'] == [[0, 2], [1]] and conf.last['reorient'] == [((0, 1, 2), (False, False, False)), None]
    assert tuple(x.shape) == (24, 24, 40, 3) and list(orig) == list(SRC)
    xs = x[:SRC[0], :SRC[1], :SRC[2]].cpu().numpy()
    assert np.array_equal(xs[..., 0], a) and np.array_equal(xs[..., 2], c)
    shape, _, mats = conform_ref.plan([SRC, b.shape, SRC], [LPS, other, LPS])
    assert shape == SRC and conform_ref.near_a_decision(mats[1], SRC, b.shape, 3).mean() <= 1e-3
    near = conform_ref.near_a_decision(mats[1], SRC, b.shape, 3)
    fov = conform_ref.inside(mats[1], SRC, b.shape)
    assert 0.3 < fov.mean() < 1.0
    ref = conform_ref.affine_resample(b[..., None], mats[1], SRC, 3, np.float64)[..., 0]
    r32 = max_dev(conform_ref.affine_resample(b[..., None], mats[1], SRC, 3, np.float32)[..., 0], ref)
    err = max_dev(xs[..., 1][~near], ref[~near])
    print('shifted modality: kernel max dev %.3g, float32 restatement %.3g, ratio %.2f' % (err, r32, err / r32))
    assert err <= 4.0 * r32
    assert np.array_equal(m[:SRC[0], :SRC[1], :SRC[2]].cpu().numpy(), zoom_ref.brain_mask(xs))   # from the pass over the finished volume
    outside = torch.ones(tuple(x.shape[:3]), dtype=torch.bool, device=dev())
    outside[:SRC[0], :SRC[1], :SRC[2]] = False
    assert float(x[outside].abs().max()) == 0.0 and float(m[outside].abs().max()) == 0.0


# ---- segment_case(geometry=...) ----
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


def scan_like(vol, seed):
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in vol], indexing='ij')
    rng = np.random.default_rng(seed)
    tex = 0.65 + 0.35 * np.sin(5.0 * g[0] + 1.0) * np.cos(4.0 * g[1] + 2.0) * np.sin(6.0 * g[2] + 0.5) + 0.02 * rng.standard_normal(vol)
    chans = []
    for c, a in enumerate((160.0, 190.0)):
        r2 = ((g[0] - 0.05 * c) / 0.3) ** 2 + (g[1] / 0.25) ** 2 + (g[2] / 0.35) ** 2
        chans.append(np.where(r2 < 1.0, 0.0, tex * a))
    return np.stack(chans, axis=-1).astype(np.float32)


def test_segment_case_with_geometry():
    """a small random model on an odd extent that pads to 16^3, the smoke run's size: on an LPS 1 mm scan the geometry path is the plain
    call bit for bit; on the same scan stored as RAS it gives the same labels, reoriented"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    from bts_amd.model import Model
    kw, vol, res = dict(base_filters=8, groups=2, reduction=2, depth=3), (13, 9, 15), 8
    padded = tuple(s + res - s % res for s in vol)
    model = Model(**kw)
    model.build((1,) + padded + (2,))
    model.set_weights_from(randomised_params(R.default_config(**kw), padded, seed=5))
    x = scan_like(vol, 4)
    stage = infer.StageSpec(model, torch.tensor([95.0, 110.0]), torch.tensor([35.0, 45.0]), res)
    y0, lab0, st0 = infer.segment_case(stage, torch.from_numpy(x).to(dev()), (1.0, 1.0, 1.0), return_stages=True)
    print('labels: %d of %d voxels are tumour' % (int((lab0 > 0).sum()), lab0.numel()))
    assert not torch.equal(y0, torch.flip(y0, (0, 1)))                                # the reorientation below is no identity on it
    conf = infer.Conformer('LPS')
    vols = [x[..., 0], x[..., 1]]
    y1, lab1, st1 = infer.segment_case(stage, None, None, geometry=(conf, vols, [LPS, LPS]), return_stages=True)
    assert conf.identity
    assert torch.equal(y0, y1) and torch.equal(lab0, lab1) and torch.equal(st0['x1mm'], st1['x1mm']) and torch.equal(st0['mask'], st1['mask'])
    ras = [ras_copy(v, LPS) for v in vols]
    y2, lab2, st2 = infer.segment_case(stage, None, None, geometry=(conf, [r[0] for r in ras], [r[1] for r in ras]), return_stages=True)
    assert not conf.identity and conf.last['code'] == 'RAS'
    assert torch.equal(st2['x1mm'], st0['x1mm'])                                      # the conformed scan is the LPS scan
    assert torch.equal(lab2, torch.flip(lab0, (0, 1))) and torch.equal(y2, torch.flip(y0, (0, 1)))
    y3, lab3 = infer.segment_scan(model, None, None, stage.mean, stage.std, res, geometry=(conf, [r[0] for r in ras], [r[1] for r in ras]))
    assert torch.equal(lab3, lab2) and torch.equal(y3, y2)


# ---- guard bands ----
@pytest.mark.parametrize('C,vol,perm,flip', [(3, (9, 7, 13), (2, 0, 1), (True, False, True)), (1, (5, 66, 4), (1, 2, 0), (False, True, False)),
                                             (8, (4, 5, 70), (0, 2, 1), (True, True, True)), (2, (1, 2, 3), (2, 1, 0), (False, False, True)),
                                             (5, (7, 3, 9), (1, 0, 2), (True, False, True)), (4, (6, 5, 131), (2, 1, 0), (False, True, False))])
def test_guard_bands_around_both_kernels(C, vol, perm, flip):
    """4 KB of 0xA5 on either side of every buffer the two kernels are handed, carved out of larger allocations (tests/test_guard_gpu.py's
    way): ragged tiles, odd channel counts, extents of 1, a channel slice of a wider destination, padding on some axes only"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    PAD, FILL = 4096, 0xA5
    live = []

    def guarded(shape):
        n = int(np.prod(shape)) * 4
        big = torch.full((n + 2 * PAD,), FILL, dtype=torch.uint8, device=dev())
        live.append((big, n))
        return big[PAD:PAD + n].view(torch.float32).view(shape)

    def check():
        torch.cuda.synchronize()
        for big, n in live:
            assert bool((big[:PAD] == FILL).all()) and bool((big[PAD + n:] == FILL).all()), 'a guard band was written'

    g = torch.Generator().manual_seed(13)
    xn = torch.randn(vol + (C,), generator=g)
    x = guarded(vol + (C,))
    x.copy_(xn)
    oshape = tuple(vol[p] for p in perm)
    out = guarded(oshape + (C,))
    ops.reorient3d(x, perm, flip, out=out)
    check()
    want = np.flip(np.transpose(xn.numpy(), perm + (3,)), [a for a in range(3) if flip[a]])
    assert np.array_equal(out.cpu().numpy(), want)
    # the same map as a gather, order 1, into a channel slice of a wider padded volume, one axis unpadded
    m = np.zeros((3, 4))
    for a in range(3):
        m[perm[a], a] = -1.0 if flip[a] else 1.0
        m[perm[a], 3] = vol[perm[a]] - 1 if flip[a] else 0.0
    m[:, 3] += (0.25, -0.375, 0.125)                                                     # off the grid: real taps, part of it outside
    pad = (oshape[0] + 3, oshape[1], oshape[2] + 1)
    lead = 1 if C < 8 else 0
    dst = guarded(pad + (lead + C + (1 if C < 7 else 0),))
    dst.fill_(7.0)
    mask = guarded(pad + (1,)) if lead == 0 and dst.shape[-1] == C else None
    ops.lib().call('bts_affine_resample3d', ops._p(x), vol[0], vol[1], vol[2], C, ops._p(dst), int(dst.shape[-1]), lead, ops._p(mask),
                   oshape[0], oshape[1], oshape[2], pad[0], pad[1], pad[2], (ctypes.c_double * 12)(*m.reshape(-1)), 1,
                   ops._stream())
    check()
    ref = conform_ref.affine_resample(xn.numpy(), m, oshape, 1, np.float32)
    got = dst[:oshape[0], :oshape[1], :oshape[2], lead:lead + C].cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    assert float(dst[oshape[0]:, :, :, lead:lead + C].abs().max()) == 0.0 and float(dst[:, :, oshape[2]:, lead:lead + C].abs().max()) == 0.0
    if lead:
        assert bool((dst[..., 0] == 7.0).all())
    if dst.shape[-1] > lead + C:
        assert bool((dst[..., lead + C:] == 7.0).all())
    if mask is not None:
        assert float(mask[oshape[0]:].abs().max()) == 0.0


# ---- the command ----
def test_command_with_conform(tmp_path, capsys):
    """python -m bts_amd.test --conform on one scan stored three ways: LPS, RAS (reoriented exactly) and LPS with its truth off the grid
    (reported and skipped); without the flag the LPS case gives the same mask"""
    import bts_amd  # noqa: F401
    from bts_amd import nifti
    from bts_amd import test as T
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    kw, vol, res = dict(base_filters=8, groups=2, reduction=2, depth=3), (13, 9, 15), 8
    padded = tuple(s + res - s % res for s in vol)
    model = Model(**kw)
    model.build((1,) + padded + (2,))
    model.set_weights_from(randomised_params(R.default_config(**kw), padded, seed=5))
    save_checkpoint(str(tmp_path / 'tumor'), model)
    save_train_args(str(tmp_path / 'tumor'), {'model_args': dict(kw), 'crop_size': list(padded)})
    np.save(str(tmp_path / 'tp.npy'), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                       'norm': {'mean': np.array([95.0, 110.0]).reshape(1, 1, 1, 2), 'std': np.array([35.0, 45.0]).reshape(1, 1, 1, 2)}})
    x = scan_like(vol, 4)
    seg = np.array([0, 1, 2, 4], dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, size=vol)]
    moved = LPS.copy()
    moved[2, 3] += 0.4
    for name, store, seg_affine in (('lps', lambda v: (v, LPS), None), ('ras', lambda v: ras_copy(v, LPS), None), ('zoff', lambda v: (v, LPS), moved)):
        os.makedirs(str(tmp_path / 'data' / name))
        for mod, ch in (('t1ce', 0), ('flair', 1)):
            nifti.save(str(tmp_path / 'data' / name / ('c_%s.nii.gz' % mod)), *store(x[..., ch]))
        arr, aff = store(seg)
        nifti.save(str(tmp_path / 'data' / name / 'c_seg.nii'), arr, aff if seg_affine is None else seg_affine)
    base = ['--in_locs', str(tmp_path / 'data'), '--modalities', 't1ce,flair', '--truth', 'seg', '--tumor_model', str(tmp_path / 'tumor'),
            '--tumor_prepro', str(tmp_path / 'tp.npy'), '--workers', '0']
    assert T.main(base + ['--out_loc', str(tmp_path / 'plain')]) == 0
    capsys.readouterr()
    assert T.main(base + ['--out_loc', str(tmp_path / 'conf'), '--conform']) == 0
    text = capsys.readouterr().out
    assert 'lps. Orientation LPS -> LPS, voxel size 1 x 1 x 1 mm, exact reorientation' in text
    assert 'ras. Orientation RAS -> LPS, voxel size 1 x 1 x 1 mm, exact reorientation' in text
    assert 'zoff: c_seg.nii does not lie on the grid of t1ce' in text and '2 cases segmented (2 scored)' in text
    plain, _ = nifti.load(str(tmp_path / 'plain' / 'lps' / 'mask.nii'))
    lps, hl = nifti.load(str(tmp_path / 'conf' / 'lps' / 'mask.nii'))
    ras, hr = nifti.load(str(tmp_path / 'conf' / 'ras' / 'mask.nii'))
    assert np.array_equal(lps, plain) and np.array_equal(ras, lps[::-1, ::-1]) and lps.any()
    assert np.array_equal(hl['affine'], LPS.astype(np.float32)) and np.array_equal(hr['affine'], ras_copy(seg, LPS)[1].astype(np.float32))
    rows = [r.split(',') for r in open(str(tmp_path / 'conf' / 'scores.csv')).read().strip().split('\n')]
    assert [r[0] for r in rows] == ['case', 'lps', 'ras', 'total'] and rows[1][1:] == rows[2][1:]
    assert not os.path.exists(str(tmp_path / 'conf' / 'zoff'))
