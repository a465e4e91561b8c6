"""-m gpu: csrc/prepro.hip (bts_prepro_occupancy, bts_prepro_sums, bts_prepro_crop_norm) and bts_amd.preprocess against results recorded
from the reference's own preprocessing (tests/golden/prepro_vectors.npz) and the numpy restatement tests/prepro_ref.py, whose equality
with those records tests/test_prepro_host.py proves.  No tolerance is taken from the kernels under test:

  occupancy, box, size, labels, count, file names, split     exact
  crop_norm with the RECORDED mean and std                    bit-equal: IEEE fp64 subtract and divide, one rounding to fp32
  sum x on integer-valued volumes (sets A-C), hence mean      bit-equal: integer terms below 2^53 add exactly in any order
  sum (x - mean)^2, std; sum x on set D                       relative N * 2^-52 (of sum |x| for the signed sum), N = voxels summed:
                                                              two fp64 summations of N terms, each within N * 2^-53 of the exact sum
  std on set D                                                the same bound plus the effect of the mean's own error, derived in
                                                              test_sums_and_compute_norm
  stored x end to end                                         1 fp32 ulp of the record (np.spacing there): mean and std off by
                                                              ~1e-13 relative can only move a quotient across a rounding tie.  On
                                                              set D the yardstick is prepro_ref's float64 mode, not the record: the
                                                              record carries the reference's float32 per-volume sum, whose mean is
                                                              off by ~1e-7 (test_prepro_host.py bounds that difference)
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import prepro_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(HERE, 'golden', 'prepro_vectors.npz'))
SPEC = json.loads(str(GOLDEN['spec']))
SETS = [s['set'] for s in SPEC]


def dev():
    return torch.device('cuda', 0)


def spec_of(name):
    return [s for s in SPEC if s['set'] == name][0]


@functools.lru_cache(maxsize=None)
def host_cases(name):
    return tuple((x.astype(np.float32), y.astype(np.float32)) for x, y in zip(GOLDEN[name + '_raw_x'], GOLDEN[name + '_raw_y']))


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64-mode restatement of the whole set, computed once"""
    return prepro_ref.run(list(host_cases(name)), create_val=spec_of(name)['create_val'], mode='float64')


def device_cases(name):
    return [(torch.from_numpy(x).to(dev()), torch.from_numpy(y[..., None].copy()).to(dev())) for x, y in host_cases(name)]


def windows(name):
    lo, hi = GOLDEN[name + '_lo'].tolist(), GOLDEN[name + '_hi'].tolist()
    cut = (slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
    return [(x[cut], y[cut]) for x, y in device_cases(name)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def box_of(occ, shape):
    lo, hi, off = [], [], 0
    for n in shape:
        idx = np.nonzero(occ[off:off + n])[0]
        lo.append(int(idx[0]))
        hi.append(int(idx[-1]))
        off += n
    return lo, hi


@pytest.mark.parametrize('name', SETS)
def test_occupancy_box_and_size(name):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    cases = device_cases(name)
    shape = tuple(cases[0][0].shape[:3])
    occ = torch.zeros(sum(shape), dtype=torch.int32, device=dev())
    for x, _ in cases:                                          # every case into the one buffer, one read-back
        ops.prepro_occupancy(x, occ)
    got = occ.cpu().numpy()
    want = np.concatenate([np.any([prepro_ref.occupancy(x)[ax] for x, _ in host_cases(name)], axis=0) for ax in range(3)])
    assert set(np.unique(got).tolist()) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)
    lo, hi = box_of(got, shape)
    assert lo == GOLDEN[name + '_lo'].tolist() and hi == GOLDEN[name + '_hi'].tolist()
    assert [h - l for l, h in zip(lo, hi)] == GOLDEN[name + '_size'][:3].tolist()
    one = torch.zeros_like(occ)                                 # a single case, twice: flags of that case alone, bitwise repeatable
    ops.prepro_occupancy(cases[0][0], one)
    two = torch.zeros_like(occ)
    ops.prepro_occupancy(cases[0][0], two)
    assert torch.equal(one, two)
    assert np.array_equal(one.cpu().numpy().astype(bool), np.concatenate(prepro_ref.occupancy(host_cases(name)[0][0])))


@pytest.mark.parametrize('shape,c', [((3, 5, 4101), 1), ((2, 3, 4098), 2), ((9, 1, 5), 16), ((1, 17, 3), 5)])
def test_occupancy_of_sparse_volumes(shape, c):
    """rows longer than one column tile (4096 planes of axis 2), the widest channel count, extents of 1; NaN counts, -0.0 does not"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(7)
    x = np.zeros(shape + (c,), np.float32)
    for _ in range(6):
        x[tuple(int(rng.integers(0, n)) for n in x.shape)] = rng.choice(np.array([1.5, -2.0, np.nan], np.float32))
    x[0, 0, shape[2] - 1, c - 1] = 3.0                          # the very last plane of axis 2
    x[tuple(int(v) for v in np.argwhere(x == 0)[-1])] = -0.0
    occ = torch.zeros(sum(shape), dtype=torch.int32, device=dev())
    ops.prepro_occupancy(torch.from_numpy(x).to(dev()), occ)
    assert np.array_equal(occ.cpu().numpy().astype(bool), np.concatenate(prepro_ref.occupancy(x)))


@pytest.mark.parametrize('name', SETS)
def test_crop_norm_with_the_recorded_statistics_is_bit_equal(name):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    mean = torch.from_numpy(GOLDEN[name + '_mean']).to(dev())
    std = torch.from_numpy(GOLDEN[name + '_std']).to(dev())
    aligned = set()
    for k, (xv, yv) in enumerate(windows(name)):
        aligned.add(xv.data_ptr() % 16 == 0)
        xo, yo = ops.prepro_crop_norm(xv, yv, mean, std)
        assert xo.is_contiguous() and yo.is_contiguous() and tuple(yo.shape) == tuple(xv.shape[:3]) + (1,)
        assert same_bits(xo.cpu().numpy(), GOLDEN[name + '_x'][k]), (name, k)
        assert same_bits(yo.cpu().numpy(), GOLDEN[name + '_y'][k]), (name, k)
        xo2, yo2 = ops.prepro_crop_norm(xv, yv, mean, std)
        assert torch.equal(xo, xo2) and torch.equal(yo, yo2)
        only_x, none = ops.prepro_crop_norm(xv, None, mean, std)
        assert none is None and torch.equal(only_x, xo)
    print('%s: window origin 16-byte aligned: %s' % (name, sorted(aligned)))
    assert aligned == ({True} if name == 'C' else {False})     # C: origin (0,0,0) and 16-byte rows; A, B, D: an origin off the grid


def test_crop_norm_row_starts_of_both_kinds():
    """one window whose rows start on and off 16-byte boundaries (row pitch 22 floats = 88 bytes); a NaN and an infinity go through
    the fp64 expression like any value"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x = host_cases('A')[0][0].copy()
    x[3, 4, 2, 0], x[3, 4, 3, 1] = np.nan, np.inf
    y = host_cases('A')[0][1]
    xg, yg = torch.from_numpy(x).to(dev()), torch.from_numpy(y[..., None].copy()).to(dev())
    cut = (slice(1, 18), slice(2, 12), slice(2, 10))
    xv, yv = xg[cut], yg[cut]
    starts = {(xv[i, j].data_ptr() % 16 == 0) for i in range(3) for j in range(4)}
    assert starts == {True, False}
    mean, std = GOLDEN['A_mean'], GOLDEN['A_std']
    xo, yo = ops.prepro_crop_norm(xv, yv, torch.from_numpy(mean).to(dev()), torch.from_numpy(std).to(dev()))
    want = ((x[cut].astype(np.float64) - mean) / std).astype(np.float32)
    got = xo.cpu().numpy()
    nan = np.isnan(want)
    assert int(nan.sum()) == 1 and np.array_equal(np.isnan(got), nan) and int(np.isinf(got).sum()) == 1
    assert same_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want))   # a NaN's payload is not specified
    assert same_bits(yo.cpu().numpy(), prepro_ref.labels(y)[cut][..., None])


def sums_of(ops, views, c, mean=None):
    acc = torch.zeros(c if mean is not None else 2 * c, dtype=torch.float64, device=dev())
    for v in views:
        ops.prepro_sums(v, acc, mean=mean)
    return acc.cpu().numpy()


@pytest.mark.parametrize('name', SETS)
def test_sums_and_compute_norm(name):
    import bts_amd  # noqa: F401
    from bts_amd import ops, preprocess
    ref = reference(name)
    c = int(GOLDEN[name + '_size'][3])
    views = [windows(name)[i][0] for i in ref['train']]
    n_vox = float(len(views) * np.prod(GOLDEN[name + '_size'][:3]))
    bound = n_vox * 2.0 ** -52
    acc = sums_of(ops, views, c)
    assert same_bits(acc[c:], ref['count'])                     # the count is exact
    crops = [prepro_ref.crop(host_cases(name)[i][0], ref['lo'], ref['hi']).astype(np.float64) for i in ref['train']]
    sum_abs = sum(np.abs(v).sum(axis=(0, 1, 2)) for v in crops)
    ratio_s = np.abs(acc[:c] - ref['sum_x']) / (bound * sum_abs)
    if name != 'D':
        assert same_bits(acc[:c], ref['sum_x'])
    assert np.all(ratio_s <= 1.0)
    mean_d = torch.from_numpy(ref['mean']).to(dev())
    q = sums_of(ops, views, c, mean=mean_d)
    ratio_q = np.abs(q - ref['sum_sq']) / (bound * ref['sum_sq'])
    print('%s: N = %d, |sum x - ref| / bound %s, |sum sq - ref| / bound %s' % (name, n_vox, ratio_s, ratio_q))
    assert np.all(ratio_q <= 1.0)
    assert same_bits(sums_of(ops, views, c), acc) and same_bits(sums_of(ops, views, c, mean=mean_d), q)   # two runs, the same bits
    mean, std = preprocess.compute_norm(views, c)
    assert mean.shape == (1, 1, 1, c) and std.shape == (1, 1, 1, c) and mean.dtype == np.float64 and std.dtype == np.float64
    if name != 'D':
        assert same_bits(mean.reshape(-1), ref['mean'])
        ratio_std = np.abs(std.reshape(-1) - ref['std']) / (bound * ref['std'])
    else:
        # mean: the sum's bound over the count, plus the division's own rounding.  std: compute_norm squares about ITS mean, m + e
        # with |e| <= dm, and  sum (x - m - e)^2 = Q - 2 e (sum x - N m) + N e^2  (sum x - N m is not 0: m divides by the count of
        # x > 0, not by N).  So Q moves by at most dq, on top of the summation bound; std = sqrt(Q / count) moves by half of that
        # relative to itself (sqrt(1 + t) <= 1 + t / 2), and the division and the square root round once each on either side:
        # 2 * (2^-54 + 2^-53) < 2^-51.
        dm = bound * sum_abs / ref['count'] + np.spacing(ref['mean'])
        assert np.all(np.abs(mean.reshape(-1) - ref['mean']) <= dm)
        dq = 2.0 * dm * np.abs(ref['sum_x'] - n_vox * ref['mean']) + n_vox * dm ** 2
        tol_std = ref['std'] * (0.5 * (bound + dq / ref['sum_sq']) + 2.0 ** -51)
        ratio_std = np.abs(std.reshape(-1) - ref['std']) / tol_std
    print('%s: |std - ref| / bound %s' % (name, ratio_std))
    assert np.all(ratio_std <= 1.0)


@pytest.mark.parametrize('c,shape,cut,shift', [(4, (6, 7, 12), (slice(1, 5), slice(0, 7), slice(2, 11)), 0),
                                               (4, (6, 7, 12), (slice(1, 5), slice(0, 7), slice(2, 11)), 1),
                                               (2, (5, 6, 9), (slice(0, 5), slice(1, 6), slice(3, 8)), 0),
                                               (2, (5, 6, 9), (slice(0, 5), slice(1, 6), slice(3, 8)), 1),
                                               (16, (3, 4, 5), (slice(1, 3), slice(0, 4), slice(1, 5)), 0),
                                               (1, (96, 97, 3), (slice(0, 96), slice(0, 97), slice(0, 3)), 0)])
def test_sums_on_every_voxel_load_path(c, shape, cut, shift):
    """C = 4 and 2 with every voxel on its 16 / 8-byte boundary (one load per voxel) and with the parent `shift` floats off it (the
    scalar path), the widest C, and 96 * 97 rows: more batches of 8 rows than the 1024 workgroups, so workgroups loop.  Values are
    integers, so the sums are exact in any order; all three kernels must read a misaligned parent correctly."""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(c * 100 + shape[2] + shift)
    x = rng.integers(-50, 900, size=shape + (c,)).astype(np.float32)
    x[rng.random(x.shape) < 0.3] = 0.0
    flat = torch.zeros(x.size + shift, dtype=torch.float32, device=dev())
    xg = flat[shift:].view(shape + (c,))
    xg.copy_(torch.from_numpy(x))
    assert xg.data_ptr() % 16 == 4 * shift
    v = xg[cut]
    acc = sums_of(ops, [v, v], c)
    w = x[cut].astype(np.float64)
    assert np.array_equal(acc[:c], 2 * w.sum(axis=(0, 1, 2))) and np.array_equal(acc[c:], 2.0 * (w > 0).sum(axis=(0, 1, 2)))
    mean = np.round(w.mean(axis=(0, 1, 2)))                     # an integer mean keeps the squares exact as well
    q = sums_of(ops, [v], c, mean=torch.from_numpy(mean).to(dev()))
    assert np.array_equal(q, ((w - mean) ** 2).sum(axis=(0, 1, 2)))
    occ = torch.zeros(sum(shape), dtype=torch.int32, device=dev())
    ops.prepro_occupancy(xg, occ)
    assert np.array_equal(occ.cpu().numpy().astype(bool), np.concatenate(prepro_ref.occupancy(x)))
    std = np.full(c, 3.0)
    xo, _ = ops.prepro_crop_norm(v, None, torch.from_numpy(mean).to(dev()), torch.from_numpy(std).to(dev()))
    assert same_bits(xo.cpu().numpy(), ((w - mean) / std).astype(np.float32))


def write_cases(root, name):
    """the fixture's raw arrays as NIfTI files; folder names count in the recorded visiting order, so sorted order reproduces it"""
    from bts_amd import nifti
    sp = spec_of(name)
    loc = os.path.join(str(root), 'scans_' + name)
    os.mkdir(loc)
    for k, (x, y) in enumerate(zip(GOLDEN[name + '_raw_x'], GOLDEN[name + '_raw_y'])):
        d = os.path.join(loc, 'case_%02d' % k)
        os.mkdir(d)
        for ch, m in enumerate(sp['modalities']):
            nifti.save(os.path.join(d, 'case_%02d_%s.nii.gz' % (k, m)), np.ascontiguousarray(x[..., ch]), np.eye(4))
        nifti.save(os.path.join(d, 'case_%02d_%s.nii.gz' % (k, sp['truth'])), y, np.eye(4))
    return loc


@pytest.mark.parametrize('name', SETS)
def test_preprocess_end_to_end(name, tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    from bts_amd.data import prepare_dataset
    sp, ref = spec_of(name), reference(name)
    loc = write_cases(tmp_path, name)
    out = os.path.join(str(tmp_path), 'data')
    r = preprocess.preprocess([loc], sp['modalities'], sp['truth'], out, create_val=sp['create_val'], device=dev(), workers=2)
    n_val = int(GOLDEN[name + '_n_val'])
    n = len(GOLDEN[name + '_x'])
    size = dict(zip('hwdc', GOLDEN[name + '_size'].tolist()))
    assert r['size'] == size and r['n_val'] == n_val and r['n_train'] == n - n_val
    assert sorted(os.listdir(out)) == ['prepro.npy', 'train', 'val']
    assert sorted(os.listdir(os.path.join(out, 'train'))) == sorted('%d.npz' % i for i in range(1, n - n_val + 1))
    assert sorted(os.listdir(os.path.join(out, 'val'))) == sorted('%d.npz' % i for i in range(1, n_val + 1))
    p = np.load(os.path.join(out, 'prepro.npy'), allow_pickle=True).item()
    assert sorted(p) == ['norm', 'size'] and p['size'] == size and sorted(p['norm']) == ['mean', 'std']
    assert p['norm']['mean'].shape == (1, 1, 1, size['c']) and same_bits(p['norm']['mean'], r['mean']) and same_bits(p['norm']['std'], r['std'])
    got_size, mean, std = preprocess.load_prepro(os.path.join(out, 'prepro.npy'))
    assert got_size == tuple(GOLDEN[name + '_size'].tolist())
    n_vox = float((n - n_val) * np.prod(GOLDEN[name + '_size'][:3]))
    if name != 'D':
        assert same_bits(mean, GOLDEN[name + '_mean'])
        assert np.all(np.abs(std - GOLDEN[name + '_std']) <= n_vox * 2.0 ** -52 * GOLDEN[name + '_std'])
    else:   # the reference's float32 running sum per volume: within n * 2^-24 * sum|x| of ours; negative values are < 1e-3 of sum|x|
        per_volume = float(np.prod(GOLDEN[name + '_size'][:3]))
        assert np.all(np.abs(mean - GOLDEN['D_mean']) <= 1.001 * per_volume * 2.0 ** -24 * np.abs(GOLDEN['D_mean']))
    worst = 0.0
    for k in range(n):
        folder, i = ('val', k + 1) if k < n_val else ('train', k - n_val + 1)
        z = np.load(os.path.join(out, folder, '%d.npz' % i))
        assert sorted(z.files) == ['x', 'y'] and z['x'].dtype == np.float32 and z['y'].dtype == np.float32
        assert z['x'].shape == GOLDEN[name + '_x'][k].shape and z['y'].shape == GOLDEN[name + '_y'][k].shape
        assert same_bits(z['y'], GOLDEN[name + '_y'][k])
        # set D: the record carries the reference's float32 per-volume sum (its mean is off by ~1e-7), so the float64 restatement
        # is the yardstick there; tests/test_prepro_host.py ties the two together
        want = GOLDEN[name + '_x'][k] if name != 'D' else ref['x'][k]
        ulps = np.abs(z['x'].astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        assert float(ulps.max()) <= 1.0, (name, k)
    print('%s: stored x, worst deviation from the record %.2f fp32 ulp' % (name, worst))
    if name == 'A':
        ds, count = prepare_dataset(os.path.join(out, 'train'), 2, got_size, (8, 8, 8), 3, device=dev(), rank=0, world=1)
        assert count == 5 and len(ds) == 3
        shapes = [(tuple(xb.shape), tuple(yb.shape)) for xb, yb in ds]
        assert shapes == [((2, 8, 8, 8, 2), (2, 8, 8, 8, 3))] * 2 + [((1, 8, 8, 8, 2), (1, 8, 8, 8, 3))]


def test_create_dataset_refuses_what_the_reference_cannot_crop(tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import nifti, preprocess
    loc = write_cases(tmp_path, 'B')
    x, y, size = preprocess.create_dataset([loc], ['t1'], 'seg', device=dev(), workers=1)
    assert len(x) == 3 and tuple(x[0].shape) == (8, 7, 7, 1) and tuple(y[0].shape) == (8, 7, 7, 1) and size == dict(h=8, w=7, d=7, c=1)
    assert x[0].is_cuda and not x[0].is_contiguous()            # views of the resident raw volumes
    assert float(y[0].max()) >= 4.0 and float(preprocess.remap_labels(y[0]).max()) == 3.0
    empty = os.path.join(loc, 'case_01', 'case_01_t1.nii.gz')
    nifti.save(empty, np.zeros((12, 10, 9), np.int16), np.eye(4))
    with pytest.raises(ValueError, match='case_01'):
        preprocess.create_dataset([loc], ['t1'], 'seg', device=dev())
    nifti.save(empty, np.ones((12, 10, 8), np.int16), np.eye(4))
    with pytest.raises(ValueError, match='case_01'):
        preprocess.create_dataset([loc], ['t1'], 'seg', device=dev())
    flat = os.path.join(str(tmp_path), 'flat')
    os.makedirs(os.path.join(flat, 'only'))
    v = np.zeros((6, 5, 4), np.int16)
    v[2, 1:4, 1:3] = 9                                          # one occupied plane of axis 0: the box has extent 0 there
    nifti.save(os.path.join(flat, 'only', 'only_t1.nii.gz'), v, np.eye(4))
    nifti.save(os.path.join(flat, 'only', 'only_seg.nii.gz'), v, np.eye(4))
    with pytest.raises(ValueError, match='zero extent'):
        preprocess.create_dataset([flat], ['t1'], 'seg', device=dev())


def test_views_that_are_not_spatial_slices_are_refused():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x = torch.zeros((6, 6, 6, 4), device=dev())
    acc = torch.zeros(8, dtype=torch.float64, device=dev())
    m = torch.ones(4, dtype=torch.float64, device=dev())
    bad = [x[..., :2], x[:, :, ::2], x.permute(1, 0, 2, 3), x.permute(0, 1, 3, 2), x.cpu(), x.double(), x[0]]
    for v in bad:
        with pytest.raises(ValueError):
            ops.prepro_sums(v, acc)
        with pytest.raises(ValueError):
            ops.prepro_crop_norm(v, None, m, m)
    with pytest.raises(ValueError):
        ops.prepro_occupancy(x[1:], torch.zeros(18, dtype=torch.int32, device=dev()))       # 17 planes
    with pytest.raises(ValueError):
        ops.prepro_occupancy(x[:, 1:], torch.zeros(17, dtype=torch.int32, device=dev()))   # a window, not a dense volume
    for occ in (None, [0] * 18, np.zeros(18, np.int32)):
        with pytest.raises(ValueError):
            ops.prepro_occupancy(x, occ)                        # not a tensor
    with pytest.raises(ValueError):
        ops.prepro_sums(x, acc.float())
    with pytest.raises(ValueError):
        ops.prepro_sums(x, acc, mean=m)                          # acc of 2C values where the second pass takes C
    with pytest.raises(ValueError):
        ops.prepro_crop_norm(x, torch.zeros((6, 6, 6, 2), device=dev())[..., :1], m, m)   # labels with a voxel stride of 2
    with pytest.raises(ValueError):
        ops.prepro_crop_norm(x, None, m.float(), m)
