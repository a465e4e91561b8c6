"""CPU: the host side of segmenting a folder of scans (bts_amd.test, infer.label_scores / scores_from_confusion) and the argument
validation of the two entry points of csrc/segment.hip.  No kernel runs here; the device side is tests/test_segment_gpu.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import segment_ref as S  # noqa: E402

import bts_amd  # noqa: E402,F401
from bts_amd import infer, nifti  # noqa: E402
from bts_amd import test as T  # noqa: E402

REQUIRED = ['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--tumor_prepro', 'p.npy', '--tumor_model', 'm']


def test_parser_defaults_are_the_references():
    """args.py:199-235, the values written out"""
    a = T.parse_args(REQUIRED)
    assert a.in_locs == ['a', 'b'] and a.modalities == ['t1ce', 'flair']
    assert a.tumor_prepro == 'p.npy' and a.tumor_model == 'm'
    assert a.truth == '' and a.skull_prepro == '' and a.skull_model == ''
    assert a.order == 3 and a.mode == 'reflect'
    assert a.spatial_tta is True and a.channel_tta == 0 and a.threshold == 0.5 and a.gpu is False
    assert a.skull_strip is False
    # ours
    assert a.dtype == 'float32' and a.tta_batch is None and a.workers == 8 and a.out_loc == ''
    b = T.parse_args(REQUIRED + ['--gpu', '--skull_model', 's', '--skull_prepro', 'q.npy', '--dtype', 'float16', '--workers', '0',
                                 '--out_loc', 'o', '--truth', 'seg', '--threshold', '0.25', '--tta_batch', '2'])
    assert b.gpu is True and b.skull_strip is True and b.dtype == 'float16' and b.workers == 0 and b.out_loc == 'o'
    assert b.truth == 'seg' and b.threshold == 0.25 and b.tta_batch == 2
    for missing in ('--in_locs', '--modalities', '--tumor_prepro', '--tumor_model'):
        i = REQUIRED.index(missing)
        with pytest.raises(SystemExit):
            T.parse_args(REQUIRED[:i] + REQUIRED[i + 2:])
    with pytest.raises(SystemExit):
        T.parse_args(REQUIRED + ['--dtype', 'int8'])


@pytest.mark.parametrize('thr', ['0', '1', '1.5', '-0.1'])
def test_threshold_must_be_a_probability(thr):
    with pytest.raises(AssertionError, match=r'Threshold must be a probability between \(0, 1\)\.'):
        T.parse_args(REQUIRED + ['--threshold', thr])


def test_skull_model_needs_skull_prepro():
    with pytest.raises(AssertionError, match='Need skull preprocessing stats if model is provided.'):
        T.parse_args(REQUIRED + ['--skull_model', 's'])
    assert T.parse_args(REQUIRED + ['--skull_prepro', 'q.npy']).skull_strip is False      # stats alone are harmless


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=1e-14, abs=0.0)


def check_scores(truth, pred, k):
    got = infer.scores_from_confusion(S.confusion(truth, pred, k))
    ref = S.scores_onehot(truth, pred, k)
    assert np.array_equal(got['confusion'], S.confusion(truth, pred, k)) and got['confusion'].dtype == np.int64
    keys = ['macro', 'micro'] + (['wt', 'tc', 'et'] if k == 4 else [])
    assert set(got) == set(keys) | {'confusion', 'dice'}
    for key in keys:
        assert same(got[key], ref[key]), (key, got[key], ref[key])
    assert len(got['dice']) == k - 1
    for c in range(k - 1):
        assert same(got['dice'][c], ref['dice'][c]), (c, got['dice'][c], ref['dice'][c])
    return got


def test_scores_from_confusion_equal_the_onehot_computation():
    rng = np.random.default_rng(7)
    lab = np.array([0, 1, 2, 4], dtype=np.uint8)
    truth = lab[rng.integers(0, 4, size=(9, 7, 5))]
    pred = np.where(rng.random(truth.shape) < 0.7, truth, lab[rng.integers(0, 4, size=truth.shape)]).astype(np.uint8)
    got = check_scores(truth, pred, 4)
    assert 0.0 < got['micro'] < 0.5 < got['macro'] < 1.0          # micro keeps util.py:55's missing factor 2
    assert got['et'] == got['dice'][2]
    check_scores(truth, pred, 2)                                   # K = 2: every label >= 1 is the one foreground class
    check_scores(truth, pred, 8)
    same_map = check_scores(truth, truth, 4)
    assert same_map['dice'] == [1.0, 1.0, 1.0] and same_map['micro'] == 0.5 and same_map['wt'] == same_map['tc'] == 1.0


def test_scores_of_empty_classes_are_nan():
    truth = np.zeros((4, 4, 4), dtype=np.uint8)
    pred = np.zeros((4, 4, 4), dtype=np.uint8)
    truth[0, 0, :3] = 1
    pred[0, 0, 1:4] = 1
    got = check_scores(truth, pred, 4)                             # classes 2 and 3 are empty in both maps
    assert got['dice'][0] == pytest.approx(2.0 * 2 / 6) and math.isnan(got['dice'][1]) and math.isnan(got['dice'][2])
    assert math.isnan(got['et']) and got['wt'] == got['tc'] == got['dice'][0]
    assert got['macro'] == pytest.approx((5.0 / 7.0 + 1.0 + 1.0) / 3.0)
    empty = check_scores(np.zeros(10, np.uint8), np.zeros(10, np.uint8), 4)
    assert math.isnan(empty['micro']) and empty['macro'] == 1.0 and all(math.isnan(v) for v in empty['dice'])
    with pytest.raises(ValueError, match='K x K'):
        infer.scores_from_confusion(np.zeros((3, 4)))


def test_label_scores_shape_mismatch_raises_with_both_shapes():
    with pytest.raises(ValueError, match=r'\(4, 5, 6\).*\(4, 5, 7\)'):
        infer.label_scores(np.zeros((4, 5, 6), np.uint8), np.zeros((4, 5, 7), np.uint8))
    with pytest.raises(ValueError, match=r'\(2, 3\).*\(3, 2\)'):
        infer.label_scores(torch.zeros((2, 3), dtype=torch.uint8), torch.zeros((3, 2), dtype=torch.uint8))


def test_entry_points_validate_before_any_hip_call():
    """BTS_ERR_SHAPE (-1) with NULL pointers and no GPU"""
    from bts_amd._lib import lib
    L = lib()

    def strip(da=8, ha=8, wa=8, d=5, h=6, w=7, db=8, hb=8, wb=8, c=2):
        return L._bts_skull_strip(None, None, None, None, None, da, ha, wa, d, h, w, db, hb, wb, c, None)

    assert strip(c=0) == -1 and strip(c=-3) == -1
    for name in ('da', 'ha', 'wa', 'd', 'h', 'w', 'db', 'hb', 'wb'):
        assert strip(**{name: 0}) == -1, name
        assert strip(**{name: -4}) == -1, name
    assert strip(d=9) == -1 and strip(h=9) == -1 and strip(w=9) == -1          # larger than both padded extents
    assert strip(da=4) == -1 and strip(hb=5) == -1 and strip(wb=6) == -1      # larger than one of them
    for k in (-1, 0, 1, 9, 64):
        assert L._bts_label_confusion(None, None, 10, k, None, None) == -1, k
    assert L._bts_label_confusion(None, None, -1, 4, None, None) == -1
    for k in (2, 4, 8):
        assert L._bts_label_confusion(None, None, 0, k, None, None) == 0      # nvox == 0: nothing to do, nothing launched


# ---- case discovery and the output layout, with the device side stubbed -------------------------------------------------------------
def write_case(folder, vol, seed, affine, names=('t1ce', 'flair'), seg=True):
    os.makedirs(folder)
    x = S.scan_like(vol, seed)
    for c, name in enumerate(names):
        nifti.save(os.path.join(folder, 'scan_%s.nii.gz' % name), x[..., c], affine)
    y = None
    if seg:
        y = np.array([0, 1, 2, 4], dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=vol)]
        nifti.save(os.path.join(folder, 'scan_seg.nii.gz'), y, affine)
    return x, y


@pytest.fixture
def stubbed(monkeypatch):
    """the command with no device: segment_case thresholds channel 0 into labels, label_scores counts with numpy"""
    seen = {'pixdim': [], 'stages': []}

    def segment_case(tumor, image, pixdim, skull=None, order=3, return_stages=False):
        seen['pixdim'].append(tuple(round(v, 4) for v in pixdim))
        seen['stages'].append((tumor, skull))
        lab = torch.where(image[..., 0] > 100.0, 4, 0) + torch.where(image[..., 1] > 130.0, 1, 0) * (image[..., 0] <= 100.0)
        return None, lab.to(torch.uint8)

    def label_scores(truth, pred, n_classes=4):
        return infer.scores_from_confusion(S.confusion(truth.cpu().numpy(), pred.cpu().numpy(), n_classes))

    monkeypatch.setattr(T, 'require_gpu', lambda: torch.device('cuda', 0) if torch.cuda.is_available() else torch.device('cpu'))
    monkeypatch.setattr(T, 'load_stage', lambda folder, prepro, args, shape: ('stage', folder, prepro, tuple(shape)))
    monkeypatch.setattr(T, 'segment_case', segment_case)
    monkeypatch.setattr(T, 'label_scores', label_scores)
    return seen


def test_cases_outputs_and_scores_with_out_loc(tmp_path, stubbed, capsys):
    data = tmp_path / 'data'
    vol = (6, 5, 7)
    aff = np.diag([1.2, 1.0, 0.9, 1.0])
    xa, ya = write_case(str(data / 'caseA'), vol, 1, np.eye(4))
    write_case(str(data / 'caseB'), vol, 2, np.eye(4), names=('t1ce',))            # flair is missing
    xc, _ = write_case(str(data / 'caseC'), vol, 3, aff, seg=False)
    xd, yd = write_case(str(data / 'caseD'), vol, 4, aff)
    outs = []
    for workers in (0, 2):
        out = tmp_path / ('out%d' % workers)
        rc = T.main(['--in_locs', str(data), '--modalities', 't1ce,flair', '--truth', 'seg', '--tumor_prepro', 'tp.npy',
                     '--tumor_model', 'tm', '--skull_model', 'sm', '--skull_prepro', 'sp.npy', '--workers', str(workers),
                     '--out_loc', str(out)])
        assert rc == 0
        outs.append(out)
    text = capsys.readouterr().out
    assert 'caseB: no *flair*.nii* file, case skipped' in text
    assert '3 cases segmented (2 scored)' in text and '1 skipped for a missing modality: caseB (flair)' in text
    assert text.count('caseA. Macro: ') == 2 and text.count('caseD. Macro: ') == 2 and 'caseC. Macro' not in text
    # the models are loaded once per run, at the first case's extent; the pixdim handed on is (dx,dy,dz) averaged over the modalities
    assert stubbed['stages'][0] == (('stage', 'tm', 'tp.npy', vol), ('stage', 'sm', 'sp.npy', vol))
    assert stubbed['pixdim'][:3] == [(1.0, 1.0, 1.0), (1.2, 1.0, 0.9), (1.2, 1.0, 0.9)]
    for out in outs:
        assert sorted(os.listdir(str(out))) == ['caseA', 'caseC', 'caseD', 'scores.csv']
        for case in ('caseA', 'caseC', 'caseD'):
            assert os.listdir(str(out / case)) == ['mask.nii']
        assert not os.path.exists(str(data / 'caseA' / 'mask.nii'))
    for case, x, a in (('caseA', xa, np.eye(4)), ('caseC', xc, aff), ('caseD', xd, aff)):
        b0, b1 = (open(str(o / case / 'mask.nii'), 'rb').read() for o in outs)
        assert b0 == b1
        lab, hdr = nifti.load(str(outs[0] / case / 'mask.nii'))
        assert lab.shape == vol and lab.dtype == np.uint8 and set(np.unique(lab).tolist()) <= {0, 1, 2, 4}
        assert np.array_equal(lab, np.where(x[..., 0] > 100.0, 4, np.where(x[..., 1] > 130.0, 1, 0)))    # the scan's own axis order
        assert np.allclose(hdr['affine'], a)
    csv0, csv1 = (open(str(o / 'scores.csv')).read() for o in outs)
    assert csv0 == csv1
    rows = [r.split(',') for r in csv0.strip().split('\n')]
    assert rows[0] == ['case', 'macro', 'micro', 'dice_1', 'dice_2', 'dice_3', 'wt', 'tc', 'et']
    assert [r[0] for r in rows[1:]] == ['caseA', 'caseD', 'total']
    conf = np.zeros((4, 4), dtype=np.int64)
    for row, case, y in ((rows[1], 'caseA', ya), (rows[2], 'caseD', yd)):
        lab = nifti.load(str(outs[0] / case / 'mask.nii'))[0]
        assert row == T.score_row(case, infer.scores_from_confusion(S.confusion(y, lab, 4)))
        conf += S.confusion(y, lab, 4)
    assert rows[3] == T.score_row('total', infer.scores_from_confusion(conf))


def test_mask_goes_into_the_case_folder_without_out_loc(tmp_path, stubbed):
    data = tmp_path / 'data'
    write_case(str(data / 'only'), (4, 5, 6), 5, np.eye(4), seg=False)
    r = T.run(T.parse_args(['--in_locs', str(data), '--modalities', 't1ce,flair', '--tumor_prepro', 'tp.npy', '--tumor_model', 'tm',
                            '--workers', '0']))
    assert r['cases'] == 1 and r['scored'] == 0 and r['skipped'] == [] and r['total'] is None
    assert stubbed['stages'] == [(('stage', 'tm', 'tp.npy', (4, 5, 6)), None)]
    assert nifti.load(str(data / 'only' / 'mask.nii'))[0].shape == (4, 5, 6)
    assert not os.path.exists(str(data / 'scores.csv'))


def test_no_gpu_ends_with_the_interpolators_message(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        T.main(['--in_locs', str(tmp_path), '--modalities', 't1ce', '--tumor_prepro', 'tp.npy', '--tumor_model', 'tm'])
