"""-m gpu: infer.StageEnsemble through infer.segment_case on tiny models (built as tests/test_segment_gpu.py builds them), the uncertainty
maps on the scan's own grid, and `python -m bts_amd.test --tumor_model A,B,C --uncertainty ...` end to end.

The mean over M members is held to the float64 mean of the single-model probabilities within mean_bound(M) of
tests/test_ensemble_kernels_gpu.py (its docstring derives it: v ((M + 1) / 2 + 2) with v = 2^-25, 1.2e-7 at M = 3), and to the float32
numpy recurrence bit for bit; labels are compared outside the voxels whose best probability lies within that bound of the threshold or of
the runner-up."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ensemble_ref as E  # noqa: E402
import segment_ref as S  # noqa: E402
import zoom_ref  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

TUMOR_KW = dict(base_filters=8, groups=2, reduction=2, depth=3)
VOL, RES = (11, 9, 14), 8
STATS = ([60.0, 70.0], [30.0, 40.0])
SEEDS = (25, 41, 57)                                      # three members: the same architecture, different weights
UNIT = (1.0, 1.0, 1.0)
PIXDIM = tuple(float(np.float32(v)) for v in (1.2, 1.0, 0.9))      # as a NIfTI header holds it


def mean_bound(m):
    return 2.0 ** -25 * ((m + 1) / 2.0 + 2.0)


def dev():
    return torch.device('cuda', 0)


def build_stage(seed, shape_padded, **kw):
    from bts_amd import infer
    from bts_amd.model import Model
    m = Model(**TUMOR_KW)
    m.build((1,) + tuple(shape_padded) + (2,))
    m.set_weights_from(S.randomised_params(R.default_config(**TUMOR_KW), tuple(shape_padded), seed))
    return infer.StageSpec(m, torch.tensor(STATS[0]), torch.tensor(STATS[1]), RES, **kw)


@pytest.fixture(scope='module')
def members():
    import bts_amd  # noqa: F401
    return [build_stage(seed, S.padded(VOL, RES)) for seed in SEEDS]


@pytest.fixture(scope='module')
def scan():
    return S.scan_like(VOL, 5)


def single(stage, x, pixdim, **kw):
    """one member through segment_case -> (y, lab, stages, its unmasked mean probability on the padded 1 mm^3 grid as numpy)"""
    from bts_amd import infer
    y, lab, st = infer.segment_case(stage, x, pixdim, return_stages=True, **kw)
    return y, lab, st, stage._tta._prob[0].cpu().numpy().copy()


@pytest.mark.parametrize('pixdim,window', [(UNIT, False), (PIXDIM, False), (UNIT, True)])
def test_an_ensemble_of_one_is_that_model_bit_for_bit(members, scan, pixdim, window):
    from bts_amd import infer
    kw = {'window': infer.WindowSpec((8, 8, 8), overlap=0.5)} if window else {}
    y0, lab0, st0, _ = single(members[0], scan, pixdim, **kw)
    ens = infer.StageEnsemble([members[0]])
    y1, lab1, st1 = infer.segment_case(ens, scan, pixdim, return_stages=True, **kw)
    assert torch.equal(y0, y1) and torch.equal(lab0, lab1) and torch.equal(st0['prob_1mm'], st1['prob_1mm'])
    assert set(st1) == set(st0) and 'uncertainty' not in st1             # no map asked for: no new key
    assert len(np.unique(lab1.cpu().numpy())) >= 3
    if window:
        assert ens.window_counts == members[0].window_counts and ens.window_counts[0] > 1
    else:
        y2, lab2 = infer.segment_scan(ens, scan, pixdim, None, None, None)            # ... and through segment_scan
        assert torch.equal(y0, y2) and torch.equal(lab0, lab2)


def test_three_members_give_the_mean_of_their_probabilities(members, scan):
    from bts_amd import infer
    probs = [single(s, scan, UNIT)[3] for s in members]
    assert float(np.abs(probs[0] - probs[1]).max()) > 0.05               # the members do differ
    ens = infer.StageEnsemble(members)
    y, lab, st = infer.segment_case(ens, scan, UNIT, return_stages=True)
    mean = ens._tta._prob[0].cpu().numpy()
    exact, _ = E.exact_moments(probs)
    err = float(np.abs(mean - exact).max())
    print('ensemble mean: max |device - fp64| %.3e (bound %.3e)' % (err, mean_bound(3)))
    assert err <= mean_bound(3)
    assert np.array_equal(mean.view(np.uint32), E.welford(probs, np.float32)[0].view(np.uint32))
    d, h, w = VOL
    mask = st['mask'].cpu().numpy()[:d, :h, :w].astype(np.float64)
    masked = exact[:d, :h, :w] * mask
    assert float(np.abs(y.cpu().numpy() - masked).max()) <= mean_bound(3)
    amb = S.ambiguous(masked, 0.5, mean_bound(3))
    got, ref = lab.cpu().numpy(), S.labels(masked, mask, 0.5)
    print('labels: %d of %d ambiguous, %d differ' % (int(amb.sum()), amb.size, int((got != ref).sum())))
    assert got.shape == VOL and int(((got != ref) & ~amb).sum()) == 0 and len(np.unique(got)) >= 3
    assert not np.array_equal(got, single(members[0], scan, UNIT)[1].cpu().numpy())              # not simply the first member's


def test_a_regions_ensemble_is_decoded_by_region_finish(scan):
    from bts_amd import infer, ops
    regs = [build_stage(seed, S.padded(VOL, RES), targets='regions') for seed in SEEDS[:2]]
    ens = infer.StageEnsemble(regs, 'entropy')
    assert ens.targets == 'regions'
    y, lab, st = infer.segment_case(ens, scan, UNIT, return_stages=True)
    tta = ens._tta
    _, want = ops.region_finish(tta._prob, tta._mask, 0.5, want_probabilities=False)
    _, argmax = ops.tta_finish(tta._prob, tta._mask, 0.5, want_probabilities=False)
    d, h, w = VOL
    assert torch.equal(lab, want[0, :d, :h, :w]) and not torch.equal(lab, argmax[0, :d, :h, :w])
    assert tuple(st['uncertainty'].shape) == VOL + (3,) and st['uncertainty'].dtype == torch.uint8


def check_levels(got, scaled, mask, what):
    ref = E.levels(scaled, mask)
    band = E.near_half(scaled)
    diff = got.astype(np.int32) - ref.astype(np.int32)
    print('%s: %d of %d within 1e-3 of a half-integer, %d levels differ, levels %d..%d' %
          (what, int(band.sum()), band.size, int((diff != 0).sum()), int(got.min()), int(got.max())))
    assert int(np.abs(diff).max()) <= 1, what
    assert not (diff != 0)[~band].any(), what
    assert band.mean() <= 0.01, what


@pytest.mark.parametrize('mode', ['std', 'entropy'])
def test_the_map_on_a_resampled_scan(members, scan, mode):
    """pixdim (1.2, 1.0, 0.9): the map has the scan's shape, is 0 outside the native mask, and in 'std' mode is the level of the float64
    variance of the members resampled at order 1; in 'entropy' mode the level of the probabilities the call itself hands back"""
    from bts_amd import infer
    probs = [single(s, scan, PIXDIM)[3] for s in members]
    ens = infer.StageEnsemble(members, mode)
    y, lab, st = infer.segment_case(ens, scan, PIXDIM, return_stages=True, postprocess={'min_component_voxels': 5})
    unc = st['uncertainty'].cpu().numpy()
    native_mask = st['uncertainty_mask'].cpu().numpy()
    assert unc.shape == VOL + (3,) and unc.dtype == np.uint8 and native_mask.shape == VOL + (1,)
    shape = infer.zoom_output_shape(VOL, PIXDIM)
    assert shape == (13, 9, 13)
    d, h, w = shape
    mback = zoom_ref.zoom(st['mask'].cpu().numpy()[:d, :h, :w].astype(np.float64), VOL, 0, np.float64)
    assert np.array_equal(native_mask, mback.astype(np.float32)) and 0.0 < mback.mean() < 1.0
    assert not unc[np.broadcast_to(native_mask == 0, unc.shape)].any() and unc[np.broadcast_to(native_mask != 0, unc.shape)].any()
    if mode == 'std':
        _, m2 = E.exact_moments([p[:d, :h, :w] for p in probs])
        var = zoom_ref.zoom(m2 / 3.0, VOL, 1, np.float64)
        check_levels(unc, E.std_scaled(var, 1.0), mback, 'std on the native grid')
    else:
        check_levels(unc, E.entropy_scaled(y.cpu().numpy()), mback, 'entropy on the native grid')
    plain = infer.segment_case(infer.StageEnsemble(members), scan, PIXDIM)                      # post-processing and the map leave
    assert torch.equal(plain[0], y)                                                             # the probabilities alone ...
    unc2 = infer.segment_case(ens, scan, PIXDIM, return_stages=True)[2]['uncertainty']
    assert torch.equal(unc2, st['uncertainty'])                                                 # ... and post-processing the map


# ---- the command -------------------------------------------------------------------------------------------------------------------
def write_case(folder, vol, seed, affine):
    from bts_amd import nifti
    os.makedirs(folder)
    x = S.scan_like(vol, seed)
    nifti.save(os.path.join(folder, 'c_t1ce.nii.gz'), x[..., 0], affine)
    nifti.save(os.path.join(folder, 'c_flair.nii'), x[..., 1], affine)
    y = np.array([0, 1, 2, 4], dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=vol)]
    nifti.save(os.path.join(folder, 'c_seg.nii.gz'), y.astype(np.int16), affine)
    return x, y


def write_model(folder, build, seed):
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    m = Model(**TUMOR_KW)
    m.build((1,) + tuple(build) + (2,))
    m.set_weights_from(S.randomised_params(R.default_config(**TUMOR_KW), tuple(build), seed))
    save_checkpoint(folder, m)
    save_train_args(folder, {'model_args': dict(TUMOR_KW), 'crop_size': list(build)})


def brain_mask(x, pixdim):
    """the mask on the scan's own grid the map is taken with: the resampled scan's positive voxels, back at order 0"""
    from bts_amd import infer
    it = infer.Interpolator(None)
    it.resample(x, pixdim, pad_res=RES)
    zeros = torch.zeros(tuple(it.mask.shape[:3]) + (3,), device=dev())
    m = it.reverse(zeros, native=True)[2][1]
    return (m > 0).to(torch.uint8).reshape(tuple(x.shape[:3])).cpu().numpy()


def test_command_with_three_checkpoints_and_entropy_maps(tmp_path, capsys):
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti
    from bts_amd import test as T
    data = tmp_path / 'data'
    cases = {'a': (write_case(str(data / 'a'), VOL, 5, np.eye(4)), UNIT),
             'b': (write_case(str(data / 'b'), VOL, 6, np.diag([1.2, 1.0, 0.9, 1.0])), PIXDIM)}
    folders = []
    for i, seed in enumerate(SEEDS):
        folders.append(str(tmp_path / ('m%d' % i)))
        write_model(folders[-1], (16, 16, 16), seed)
    np.save(str(tmp_path / 'tp.npy'), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                       'norm': {'mean': np.array(STATS[0]).reshape(1, 1, 1, 2), 'std': np.array(STATS[1]).reshape(1, 1, 1, 2)}})
    common = ['--in_locs', str(data), '--modalities', 't1ce,flair', '--truth', 'seg', '--tumor_prepro', str(tmp_path / 'tp.npy')]
    outs = []
    for workers in (0, 2):
        out = tmp_path / ('out%d' % workers)
        assert T.main(common + ['--tumor_model', ','.join(folders), '--uncertainty', 'entropy', '--workers', str(workers),
                                '--out_loc', str(out)]) == 0
        outs.append(out)
    text = capsys.readouterr().out
    assert text.count('Ensemble of 3: ') == 2 and text.count('a. Uncertainty (entropy) qu_score_class_1: ') == 2
    keys = T.uncertainty_keys('labels')
    csv0, csv1 = (open(str(o / 'scores.csv')).read() for o in outs)
    assert csv0 == csv1
    rows = [r.split(',') for r in csv0.strip().split('\n')]
    assert [r[0] for r in rows] == ['case', 'a', 'b', 'total'] and all(len(r) == 9 + 12 for r in rows) and rows[0][9:] == list(keys)
    per_case = []
    for row, case in ((rows[1], 'a'), (rows[2], 'b')):
        (x, truth), pixdim = cases[case]
        lab, hdr = nifti.load(str(outs[0] / case / 'mask.nii'))
        assert open(str(outs[0] / case / 'mask.nii'), 'rb').read() == open(str(outs[1] / case / 'mask.nii'), 'rb').read()
        chans = []
        for name in ('1', '2', '4'):
            path = [str(o / case / ('unc_%s.nii' % name)) for o in outs]
            assert open(path[0], 'rb').read() == open(path[1], 'rb').read(), (case, name)
            u, uh = nifti.load(path[0])
            assert u.dtype == np.uint8 and u.shape == VOL and int(u.max()) <= 100 and int(u.max()) > 0
            assert np.array_equal(uh['affine'], hdr['affine']) and np.array_equal(uh['pixdim'][:4], hdr['pixdim'][:4])
            chans.append(np.asarray(u))
        unc = np.ascontiguousarray(np.stack(chans, axis=-1))
        s = infer.uncertainty_scores(truth, np.ascontiguousarray(lab), unc, brain_mask(x, pixdim), 'labels')
        assert row[9:] == ['%.6f' % s[k] for k in keys], case
        assert row[:9] == T.score_row(case, infer.label_scores(truth, np.ascontiguousarray(lab)))
        per_case.append(s)
    assert rows[3][9:] == ['%.6f' % T.mean_finite([s[k] for s in per_case]) for k in keys]
    # one checkpoint and no --uncertainty: the bytes of the plain StageSpec through segment_case, and no map
    out = tmp_path / 'single'
    assert T.main(common + ['--tumor_model', folders[0], '--workers', '0', '--out_loc', str(out)]) == 0
    assert 'Ensemble of' not in capsys.readouterr().out
    args = T.parse_args(common + ['--tumor_model', folders[0]])
    stage = T.load_stage(folders[0], str(tmp_path / 'tp.npy'), args, VOL)
    assert isinstance(stage, infer.StageSpec)
    want = [['case', 'macro', 'micro', 'dice_1', 'dice_2', 'dice_3', 'wt', 'tc', 'et']]
    conf = np.zeros((4, 4), dtype=np.int64)
    for case in ('a', 'b'):
        (x, truth), pixdim = cases[case]
        assert sorted(os.listdir(str(out / case))) == ['mask.nii']
        _, lab = infer.segment_case(stage, torch.from_numpy(x).to(dev()), pixdim)
        ref = tmp_path / ('ref_%s.nii' % case)
        affine = np.mean([nifti.load(str(data / case / f))[1]['affine'] for f in ('c_t1ce.nii.gz', 'c_flair.nii')], axis=0, dtype=np.float32)
        nifti.save(str(ref), lab.cpu().numpy(), affine)
        assert open(str(ref), 'rb').read() == open(str(out / case / 'mask.nii'), 'rb').read(), case
        s = infer.label_scores(truth, lab.cpu().numpy())
        conf += s['confusion']
        want.append(T.score_row(case, s))
    want.append(T.score_row('total', infer.scores_from_confusion(conf)))
    assert open(str(out / 'scores.csv')).read() == ''.join(','.join(r) + '\n' for r in want)
