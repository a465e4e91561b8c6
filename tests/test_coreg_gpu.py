"""-m gpu: the two device passes of rigid co-registration (csrc/coreg.hip: bts_quantize_bins, bts_joint_hist_pv), `coreg.coregister` on
top of them and the command line's --coregister, against the float64 / integer restatement tests/coreg_ref.py (whose vectorised histogram
tests/test_coreg_host.py proves equal to the rule written out point by point).

There is no tolerance anywhere: the quantiser is bit-equal, the histograms are equal as integers, and a whole registration takes the same
steps with the device evaluator as with the numpy one.  The histogram's equality holds because the kernel forms its coordinate with the
same separately rounded float64 operations as the reference; tests/test_coreg_host.py also shows that no lattice point of any case used
here lies within 1e-9 of a rounding tie, so even a contracted multiply-add could not change a count.  Extents are odd and unequal (19x23x37,
17x29x21), so no two axes can be confused and a workgroup's run of 2048 lattice points ends mid-way (16169 points: eight workgroups)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import coreg_ref as R  # noqa: E402
from guard_alloc import POISON, install  # noqa: E402

pytestmark = pytest.mark.gpu

Q3 = 32 ** 3
CASES = R.hist_cases()


def dev():
    return torch.device('cuda', 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ---- bts_quantize_bins ----
@pytest.mark.parametrize('bins', [2, 32, 64])
def test_quantize_bit_equal(bins):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    lo, hi = -0.75, 1.25                                              # dyadic: the interior bin edges lo + k (hi - lo) / bins are exact
    edges = lo + (hi - lo) * np.arange(bins + 1) / bins
    special = np.concatenate([[-5.0, np.nextafter(np.float32(lo), np.float32(-9)), lo, hi, np.nextafter(np.float32(hi), np.float32(9)), 7.0],
                              edges, np.nextafter(edges.astype(np.float32), np.float32(-9)), np.nextafter(edges.astype(np.float32), np.float32(9))])
    rng = np.random.default_rng(bins)
    for shape in ((1,), (3,), (255,), (257,), (19, 23, 37)):
        n = int(np.prod(shape))
        x = (rng.random(n) * 3.0 - 1.5).astype(np.float32)
        x[:min(n, special.size)] = special[:min(n, special.size)].astype(np.float32)
        if n == 3:
            x[:] = (lo, hi, 0.25)
        x = x.reshape(shape)
        xg = up(x)
        got = ops.quantize_bins(xg, lo, hi, bins)
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape
        assert np.array_equal(got.cpu().numpy(), R.quantize(x, lo, hi, bins)), shape
        assert np.array_equal(xg.cpu().numpy(), x)
    odd = ops.quantize_bins(up(x), 0.1, 0.7, bins)                       # bounds that are no binary fractions
    assert np.array_equal(odd.cpu().numpy(), R.quantize(x, 0.1, 0.7, bins))


# ---- bts_joint_hist_pv ----
def volumes(fs, ms, bins):
    return R.binned_volume(fs, bins, 1), R.binned_volume(ms, bins, 2)


@pytest.mark.parametrize('case', range(len(CASES)), ids=[c[0] for c in CASES])
def test_joint_hist_equals_the_reference(case):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    name, fs, ms, mats = CASES[case]
    for bins in (32,) if name in ('general rigid', 'moving axis of extent 1') else (2, 32, 64):
        qf, qm = volumes(fs, ms, bins)
        gf, gm = up(qf), up(qm)
        for origin, stride, counts in R.LATTICES:
            want = R.joint_hist_pv(qf, qm, origin, stride, counts, mats, bins)
            got = ops.joint_hist_pv(gf, gm, origin, stride, counts, mats, bins)
            assert got.dtype == torch.int64 and tuple(got.shape) == (len(mats), bins, bins)
            assert np.array_equal(got.cpu().numpy(), want), (name, bins, origin, stride)
            again = ops.joint_hist_pv(gf, gm, origin, stride, counts, mats, bins)
            assert torch.equal(got, again)                                # integer sums: the same bits in every run
            npts = int(np.prod(counts))
            if name == 'identity':
                sel = tuple(slice(o, o + s * (n - 1) + 1, s) for o, s, n in zip(origin, stride, counts))
                pairs = qf[sel].astype(np.int64).reshape(-1) * bins + qm[sel].astype(np.int64).reshape(-1)
                assert np.array_equal(want[0], (np.bincount(pairs, minlength=bins * bins) * Q3).reshape(bins, bins))
                assert int(got.sum()) == npts * Q3                        # the clamped neighbour of the last plane weighs nothing
            if name == 'everything outside':
                assert int(got.abs().sum()) == 0
            if name == 'integer shift, partly outside':
                assert 0 < int(got.sum()) < npts * Q3 and int(got.sum()) % Q3 == 0
            if name == 'half-voxel shift':
                assert int((got.cpu() % (16 ** 3)).abs().sum()) == 0       # every weight is (Q / 2)^3
        assert np.array_equal(gf.cpu().numpy(), qf) and np.array_equal(gm.cpu().numpy(), qm)


def test_thirteen_candidates_equal_thirteen_calls():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    mats = R.thirteen()
    assert len({m.tobytes() for m in mats}) == 13
    qf, qm = volumes(R.FIXED, R.MOVING, 32)
    gf, gm = up(qf), up(qm)
    origin, stride, counts = R.LATTICES[1]
    all13 = ops.joint_hist_pv(gf, gm, origin, stride, counts, mats, 32)
    for k in range(13):
        assert torch.equal(all13[k], ops.joint_hist_pv(gf, gm, origin, stride, counts, mats[k:k + 1], 32)[0]), k
    assert len({all13[k].cpu().numpy().tobytes() for k in range(13)}) == 13
    assert torch.equal(all13, ops.joint_hist_pv(gf, gm, origin, stride, counts, np.concatenate([mats, np.tile([[[0, 0, 0, 1.0]]], (13, 1, 1))], axis=1), 32))


def raw_hist(L, qf, qm, lat, mats, bins, hist):
    from bts_amd import ops
    (o, s, n), m = lat, np.ascontiguousarray(mats, dtype=np.float64)
    return L._bts_joint_hist_pv(ops._p(qf), qf.shape[0], qf.shape[1], qf.shape[2], ops._p(qm), qm.shape[0], qm.shape[1], qm.shape[2],
                                o[0], o[1], o[2], s[0], s[1], s[2], n[0], n[1], n[2], (ctypes.c_double * m.size)(*m.reshape(-1)),
                                len(m), bins, ops._p(hist), ops._stream())


def test_hist_is_overwritten():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    _, fs, ms, mats = CASES[3]
    qf, qm = volumes(fs, ms, 32)
    hist = torch.full((len(mats), 32, 32), -1, dtype=torch.int64, device=dev())     # 0xFF bytes
    assert raw_hist(ops.lib(), up(qf), up(qm), R.LATTICES[0], mats, 32, hist) == 0
    assert np.array_equal(hist.cpu().numpy(), R.joint_hist_pv(qf, qm, *R.LATTICES[0], mats, 32))


@pytest.mark.parametrize('case', [0, 1], ids=['identity', 'integer shift'])
def test_guard_bands_and_poison(monkeypatch, case):
    """qf, qm and the histogram carved out of larger pattern-filled allocations (tests/guard_alloc.py; the call has no workspace); the
    coordinates of these two cases touch N - 1.  The bands stay intact, and a run on 0x00-filled memory equals one on 0xFF-filled memory"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    name, fs, ms, mats = CASES[case]
    qf, qm = volumes(fs, ms, 32)
    results = []
    for fill in (0x00, POISON):
        with monkeypatch.context() as mp:
            g = install(mp, fill)
            gf, gm = g._alloc(fs, torch.uint8, dev()), g._alloc(ms, torch.uint8, dev())
            gf.copy_(up(qf))
            gm.copy_(up(qm))
            out = [ops.joint_hist_pv(gf, gm, o, s, n, mats, 32) for o, s, n in R.LATTICES]
            x = g._alloc(fs, torch.float32, dev())
            x.copy_(up(qf.astype(np.float32)))
            out.append(ops.quantize_bins(x, 0.0, 32.0, 32))
            assert g.check() >= 3 + len(out)
            results.append([t.cpu().numpy().copy() for t in out])
    for a, b, lat in zip(results[0], results[1], R.LATTICES):
        assert np.array_equal(a, b)
        assert np.array_equal(a, R.joint_hist_pv(qf, qm, *lat, mats, 32)), name
    assert np.array_equal(results[0][-1], qf) and np.array_equal(results[1][-1], qf)


def test_refusals():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    L = ops.lib()
    qf, qm = up(np.zeros(R.FIXED, dtype=np.uint8)), up(np.zeros(R.MOVING, dtype=np.uint8))
    lat, one = R.LATTICES[0], R.shift(0, 0, 0)[None]
    good = dict(qf=qf, qm=qm, origin=lat[0], stride=lat[1], counts=lat[2], matrices=one, bins=32)
    ops.joint_hist_pv(**good)
    bad = [dict(bins=1), dict(bins=65), dict(bins=32.5), dict(origin=(-1, 0, 0)), dict(stride=(0, 1, 1)), dict(counts=(0, 23, 37)),
           dict(counts=(20, 23, 37)), dict(origin=(1, 0, 0)), dict(stride=(2, 1, 1)), dict(origin=(0, 0)), dict(matrices=np.zeros((0, 3, 4))),
           dict(matrices=np.zeros((33, 3, 4))), dict(matrices=np.zeros((1, 2, 4))), dict(matrices=np.full((1, 3, 4), np.nan)),
           dict(qf=qf.float()), dict(qm=qm.cpu()), dict(qf=qf[:, :, ::2]), dict(qf=qf[0]), dict(qm=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.joint_hist_pv(**dict(good, **kw))
    x = torch.zeros(5, device=dev())
    for args in ((x, 0.0, 1.0, 1), (x, 0.0, 1.0, 65), (x, 1.0, 1.0, 32), (x, 2.0, 1.0, 32), (x, 0.0, float('inf'), 32), (x, float('nan'), 1.0, 32),
                 (x[:0], 0.0, 1.0, 32), (x.double(), 0.0, 1.0, 32), (x[::2], 0.0, 1.0, 32), (x.cpu(), 0.0, 1.0, 32)):
        with pytest.raises(ValueError):
            ops.quantize_bins(*args)
    # the library's own checks, through the raw binding: BTS_ERR_SHAPE (-1), nothing launched
    q = torch.zeros(5, dtype=torch.uint8, device=dev())
    s = ops._stream()
    assert L._bts_quantize_bins(ops._p(x), ops._p(q), 5, 0.0, 1.0, 32, s) == 0
    for args in ((ops._p(x), ops._p(q), 0, 0.0, 1.0, 32), (ops._p(x), ops._p(q), -1, 0.0, 1.0, 32), (ops._p(x), ops._p(q), 5, 1.0, 1.0, 32),
                 (ops._p(x), ops._p(q), 5, 1.0, 0.0, 32), (ops._p(x), ops._p(q), 5, 0.0, float('inf'), 32),
                 (ops._p(x), ops._p(q), 5, float('nan'), 1.0, 32), (ops._p(x), ops._p(q), 5, float('-inf'), 1.0, 32),
                 (ops._p(x), ops._p(q), 5, 0.0, 1.0, 1), (ops._p(x), ops._p(q), 5, 0.0, 1.0, 65), (None, ops._p(q), 5, 0.0, 1.0, 32),
                 (ops._p(x), None, 5, 0.0, 1.0, 32)):
        assert L._bts_quantize_bins(*(args + (s,))) == -1, args[2:]
    hist = torch.zeros((1, 32, 32), dtype=torch.int64, device=dev())
    assert raw_hist(L, qf, qm, lat, one, 32, hist) == 0
    for o, st, n in (((-1, 0, 0), (1, 1, 1), (19, 23, 37)), ((0, 0, 0), (0, 1, 1), (19, 23, 37)), ((0, 0, 0), (1, 1, 1), (19, 0, 37)),
                     ((0, 0, 0), (1, 1, 1), (19, 23, 38)), ((0, 1, 0), (1, 1, 1), (19, 23, 37)), ((0, 0, 0), (1, 2, 1), (19, 23, 37)),
                     ((19, 0, 0), (1, 1, 1), (1, 23, 37))):
        assert raw_hist(L, qf, qm, (o, st, n), one, 32, hist) == -1, (o, st, n)
    for bins in (1, 65, 0):
        assert raw_hist(L, qf, qm, lat, one, bins, hist) == -1
    many = np.tile(one, (33, 1, 1))
    big = torch.zeros((33, 32, 32), dtype=torch.int64, device=dev())
    assert raw_hist(L, qf, qm, lat, many, 32, big) == -1 and raw_hist(L, qf, qm, lat, many[:32], 32, big) == 0
    m12 = (ctypes.c_double * 12)(*one.reshape(-1))
    dims = (19, 23, 37)

    def call(pf, df, pm, dm, m, k, h):
        return L._bts_joint_hist_pv(pf, df[0], df[1], df[2], pm, dm[0], dm[1], dm[2], 0, 0, 0, 1, 1, 1, 1, 1, 1, m, k, 32, h, s)
    assert call(ops._p(qf), dims, ops._p(qm), R.MOVING, m12, 1, ops._p(hist)) == 0
    assert call(None, dims, ops._p(qm), R.MOVING, m12, 1, ops._p(hist)) == -1
    assert call(ops._p(qf), dims, None, R.MOVING, m12, 1, ops._p(hist)) == -1
    assert call(ops._p(qf), dims, ops._p(qm), R.MOVING, None, 1, ops._p(hist)) == -1
    assert call(ops._p(qf), dims, ops._p(qm), R.MOVING, m12, 1, None) == -1
    assert call(ops._p(qf), dims, ops._p(qm), R.MOVING, m12, 0, ops._p(hist)) == -1
    assert call(ops._p(qf), (0, 23, 37), ops._p(qm), R.MOVING, m12, 1, ops._p(hist)) == -1
    assert call(ops._p(qf), dims, ops._p(qm), (17, 29, 0), m12, 1, ops._p(hist)) == -1
    assert call(ops._p(qf), (2048, 2048, 512), ops._p(qm), R.MOVING, m12, 1, ops._p(hist)) == -1       # 2^31 voxels
    torch.cuda.synchronize()


# ---- the optimiser on top of the kernel ----
@pytest.mark.parametrize('key', ['pose_a', 'same_grid'])
def test_same_trajectory_on_the_device_and_in_numpy(key):
    """coreg.coregister on device volumes, once with the device evaluator and once with the numpy one on the same binned volumes: the
    same parameters, the same number of evaluations, the same score as a float, sweep by sweep"""
    import bts_amd  # noqa: F401
    from bts_amd import coreg
    from test_coreg_host import LEVELS, POSES
    (fs, fsp), (ms, msp), pose, _ = POSES[key]
    a_f = R.grid_affine(fs, fsp)
    truth = coreg.rigid_matrix(pose, (a_f @ np.array([(n - 1) // 2 for n in fs] + [1.0]))[:3])
    f, a_f, m, a_m = R.phantom_pair(fs, fsp, ms, msp, truth, moving_offset=(1.3, -0.7, 2.1) if ms != fs else (0.0, 0.0, 0.0))
    fg, mg = up(f), up(m)
    on_device = coreg.coregister(fg, a_f, mg, a_m, levels=LEVELS)
    in_numpy = coreg.coregister(fg, a_f, mg, a_m, levels=LEVELS, evaluate=R.joint_hist_pv)
    assert on_device.params == in_numpy.params and on_device.evaluations == in_numpy.evaluations
    assert on_device.nmi_after == in_numpy.nmi_after and on_device.nmi_before == in_numpy.nmi_before
    assert on_device.trace == in_numpy.trace and on_device.overlap == in_numpy.overlap
    assert on_device.nmi_after >= on_device.nmi_before
    tre = R.mean_tre(on_device.matrix, truth, fs, a_f)
    print('%s on the device: %s, mean TRE %.4f voxel, %d evaluations' % (key, on_device.params, tre, on_device.evaluations))
    # the device's percentiles and bins are those of the host restatement
    lo, hi = coreg.percentile_bounds(np.sort(f, axis=None))
    assert np.array_equal(coreg._binned(fg, 32, 'fixed').cpu().numpy(), R.quantize(f, lo, hi, 32))


# ---- the command ----
def test_command_with_coregister(tmp_path, capsys):
    """python -m bts_amd.test --conform --coregister on a two-modality phantom whose second header is off by a known rigid motion: the
    run completes, prints what coreg.coregister_case finds for the same arrays, and writes mask.nii on the first modality's grid"""
    import bts_amd  # noqa: F401
    from bts_amd import coreg, nifti
    from bts_amd import test as T
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    from oracle import torch_ref as O
    from segment_ref import randomised_params
    fs, ms = (28, 33, 25), (24, 37, 27)
    shrink = np.diag([1.0 / 6.0] * 3 + [1.0])                             # the phantom's 6 mm world stored as 1 mm headers
    a6 = R.grid_affine(fs, (6.0,) * 3)
    truth = coreg.rigid_matrix((9.0, -6.0, 6.0, 3.0, -2.0, 4.0), (a6 @ np.array([13, 16, 12, 1.0]))[:3])
    f, a_f, m, a_m = R.phantom_pair(fs, (6.0,) * 3, ms, (6.6, 5.4, 5.8), truth)
    kw, res = dict(base_filters=8, groups=2, reduction=2, depth=3), 8
    plan_shape = fs
    padded = tuple(s + res - s % res for s in plan_shape)
    model = Model(**kw)
    model.build((1,) + padded + (2,))
    model.set_weights_from(randomised_params(O.default_config(**kw), padded, seed=5))
    save_checkpoint(str(tmp_path / 'tumor'), model)
    save_train_args(str(tmp_path / 'tumor'), {'model_args': dict(kw), 'crop_size': list(padded)})
    np.save(str(tmp_path / 'tp.npy'), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                       'norm': {'mean': np.array([0.2, 0.2]).reshape(1, 1, 1, 2), 'std': np.array([0.2, 0.2]).reshape(1, 1, 1, 2)}})
    os.makedirs(str(tmp_path / 'data' / 'one'))
    nifti.save(str(tmp_path / 'data' / 'one' / 'c_t1ce.nii.gz'), f, shrink @ a_f)
    nifti.save(str(tmp_path / 'data' / 'one' / 'c_flair.nii.gz'), m, shrink @ a_m)
    base = ['--in_locs', str(tmp_path / 'data'), '--modalities', 't1ce,flair', '--tumor_model', str(tmp_path / 'tumor'),
            '--tumor_prepro', str(tmp_path / 'tp.npy'), '--workers', '0', '--conform', 'RAS']
    assert T.main(base + ['--out_loc', str(tmp_path / 'plain')]) == 0
    assert 'Coregistered' not in capsys.readouterr().out
    assert T.main(base + ['--out_loc', str(tmp_path / 'reg'), '--coregister', '--coregister_max_mm', '4', '--coregister_bins', '16']) == 0
    text = capsys.readouterr().out
    case = T.decode_case(str(tmp_path / 'data' / 'one'), ['t1ce', 'flair'], '', True)
    vols, _ = T.upload_conform_case(case, dev())
    affines, found = coreg.coregister_case(vols, case['affines'], bounds=(4.0, 20.0), bins=16)
    assert 'one. Coregistered ' + coreg.format_result('flair', found[1]) in text
    assert found[1].nmi_after >= found[1].nmi_before and all(abs(v) <= 4.0 for v in found[1].params[:3])
    assert np.array_equal(affines[0], case['affines'][0])
    for where in ('plain', 'reg'):
        mask, hdr = nifti.load(str(tmp_path / where / 'one' / 'mask.nii'))
        assert tuple(mask.shape) == fs and np.array_equal(hdr['affine'], (shrink @ a_f).astype(np.float32))
