"""-m gpu: csrc/segment.hip (bts_skull_strip, bts_label_confusion) against numpy, infer.segment_case stage by stage against the oracle
applied to the engine's own previous-stage output, and `python -m bts_amd.test` end to end on three tiny cases."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import segment_ref as S  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

SENTINEL = -777.0


def dev():
    return torch.device('cuda', 0)


# ---- bts_skull_strip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 2, 3, 4])
@pytest.mark.parametrize('orig,pad_a,pad_b', [((5, 6, 7), (8, 8, 8), (8, 8, 8)),
                                              ((13, 9, 16), (16, 16, 24), (16, 12, 20))])
def test_skull_strip_is_bit_equal_to_numpy(c, orig, pad_a, pad_b):
    """the second case: a different resolution per stage, the second padding smaller than the first on two axes.  p leaves [0,1] and x
    is negative in places (no clamping may creep in); the outputs start as a sentinel (the padding must be WRITTEN as zero)"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(11 * c + orig[0])
    x = (rng.standard_normal(pad_a + (c,)) * 50.0).astype(np.float32)
    p = (rng.random(pad_a + (1,)) * 1.6 - 0.3).astype(np.float32)
    m = (rng.random(pad_a + (1,)) > 0.3).astype(np.float32)
    assert p.min() < 0.0 and p.max() > 1.0 and x.min() < 0.0
    xo_ref, mo_ref = S.strip(x, p, m, orig, pad_b)
    xo = torch.full(pad_b + (c,), SENTINEL, device=dev())
    mo = torch.full(pad_b + (1,), SENTINEL, device=dev())
    got = ops.skull_strip(torch.from_numpy(x).to(dev()), torch.from_numpy(p).to(dev()), torch.from_numpy(m).to(dev()), orig, pad_b,
                          out=(xo, mo))
    assert got[0] is xo and got[1] is mo
    assert np.array_equal(xo.cpu().numpy().view(np.uint32), xo_ref.view(np.uint32))
    assert np.array_equal(mo.cpu().numpy().view(np.uint32), mo_ref.view(np.uint32))
    xn, mn = ops.skull_strip(torch.from_numpy(x).to(dev()), torch.from_numpy(p).to(dev()), torch.from_numpy(m).to(dev()), orig, pad_b)
    assert torch.equal(xn, xo) and torch.equal(mn, mo)


def test_skull_strip_refuses_bad_extents():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x, p = torch.zeros((8, 8, 8, 2), device=dev()), torch.zeros((8, 8, 8, 1), device=dev())
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.skull_strip(x, p, p, (5, 6, 9), (8, 8, 16))          # unpadded extent beyond the first padding
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.skull_strip(x, p, p, (5, 6, 7), (8, 8, 4))           # ... beyond the second
    with pytest.raises(ValueError):
        ops.skull_strip(x, torch.zeros((8, 8, 8, 2), device=dev()), p, (5, 6, 7), (8, 8, 8))


# ---- bts_label_confusion ---------------------------------------------------------------------------------------------------------
def label_maps(n, seed):
    """piecewise-constant maps (runs, as along a scan row) with labels 0..4 and 255, and a pure-noise stretch"""
    rng = np.random.default_rng(seed)
    vals = np.array([0, 0, 0, 1, 2, 3, 4, 255], dtype=np.uint8)
    t = np.repeat(vals[rng.integers(0, 8, size=n // 5 + 1)], 5)[:n].copy()
    p = np.repeat(vals[rng.integers(0, 8, size=n // 7 + 1)], 7)[:n].copy()
    k = min(n, 64)
    t[:k] = vals[rng.integers(0, 8, size=k)]
    return t, p


@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('n', [1, 15, 210, 33 * 17 * 9, 2 ** 22 + 3, 2 ** 23 + 3])
def test_label_confusion_is_exact(n, k):
    """the grid is capped at 1024 workgroups of 256 lanes, one 16-voxel chunk per lane and pass: 2^22 + 3 voxels fill every lane of the
    capped grid exactly once, 2^23 + 3 send every lane round the grid-stride loop a second time"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    t, p = label_maps(n, n % 1000 + k)
    if n > 100:
        assert {3, 4, 255} <= set(np.unique(t).tolist())
    ref = S.confusion(t, p, k)
    assert int(ref.sum()) == n
    tg, pg = torch.from_numpy(t).to(dev()), torch.from_numpy(p).to(dev())
    c1 = ops.label_confusion(tg, pg, k)
    assert c1.dtype == torch.int64 and tuple(c1.shape) == (k, k)
    assert np.array_equal(c1.cpu().numpy(), ref)
    c2 = ops.label_confusion(tg, pg, k)                          # a second run: the same bytes
    assert c1.cpu().numpy().tobytes() == c2.cpu().numpy().tobytes()
    ops.label_confusion(pg, tg, k, counts=c2)                    # two calls into one buffer: the sum
    assert np.array_equal(c2.cpu().numpy(), ref + ref.T)


@pytest.mark.parametrize('off_t,off_p', [(1, 1), (3, 3), (8, 8), (3, 8), (0, 5)])
def test_label_confusion_off_a_16_byte_boundary(off_t, off_p):
    """views that start 1, 3 and 8 bytes past a 16-byte boundary (head and tail go voxel by voxel), and the two maps unequally far
    from one (byte loads)"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    n = 33 * 17 * 9
    t, p = label_maps(n + 16, 77)
    tg, pg = torch.from_numpy(t).to(dev()), torch.from_numpy(p).to(dev())
    assert tg.data_ptr() % 16 == 0 and pg.data_ptr() % 16 == 0
    for length in (n, 15, 17):
        tv, pv = tg[off_t:off_t + length], pg[off_p:off_p + length]
        assert tv.data_ptr() % 16 == off_t and pv.data_ptr() % 16 == off_p
        got = ops.label_confusion(tv, pv, 4)
        assert np.array_equal(got.cpu().numpy(), S.confusion(t[off_t:off_t + length], p[off_p:off_p + length], 4)), length


def test_label_scores_on_the_device_equal_the_onehot_computation():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    t, p = label_maps(12 * 13 * 14, 5)
    t, p = t.reshape(12, 13, 14), p.reshape(12, 13, 14)
    ref = S.scores_onehot(t, p, 4)
    for got in (infer.label_scores(t, p), infer.label_scores(torch.from_numpy(t).to(dev()), torch.from_numpy(p).to(dev()))):
        assert np.array_equal(got['confusion'], S.confusion(t, p, 4))
        for key in ('macro', 'micro', 'wt', 'tc', 'et'):
            assert got[key] == pytest.approx(ref[key], rel=1e-14)
        assert got['dice'] == pytest.approx(ref['dice'], rel=1e-14)
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        infer.label_scores(t, p, n_classes=9)


# ---- the two-stage path, stage by stage --------------------------------------------------------------------------------------------
SKULL_KW = dict(base_filters=4, groups=2, reduction=2, depth=2, out_ch=1)
TUMOR_KW = dict(base_filters=8, groups=2, reduction=2, depth=3)
VOL, SEED = (11, 9, 14), 5
# SEED was chosen on the CPU with the oracle alone (segment_ref.two_stage): of the 1386 voxels of the scan 7 are ambiguous (within 1e-4
# of the threshold or of a tie; 6 of them are masked-out voxels, a tie at 0) with pixdim (1.2, 1.0, 0.9) and 11 with (1, 1, 1): 0.51 %
# and 0.79 %, under the 1 % the comparison allows; both label maps hold all of {0, 1, 2, 4}.
SKULL_STATS = ([95.0, 110.0], [35.0, 45.0])
TUMOR_STATS = ([60.0, 70.0], [30.0, 40.0])


def engine_stage(kw, P, shape_padded, stats, res):
    from bts_amd import infer
    from bts_amd.model import Model
    m = Model(**kw)
    m.build((1,) + tuple(shape_padded) + (2,))
    m.set_weights_from(P)
    return infer.StageSpec(m, torch.tensor(stats[0]), torch.tensor(stats[1]), res)


@pytest.fixture(scope='module')
def two_stage():
    """per pixdim: the scan, the engine's result with its stages, and the oracle parameter sets (built once, never modified)"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    out = {}
    for pixdim in ((1.2, 1.0, 0.9), (1.0, 1.0, 1.0)):
        x = S.scan_like(VOL, SEED)
        unit = all(f == 1.0 for f in pixdim)
        shape = VOL if unit else infer.zoom_output_shape(VOL, pixdim)
        scfg, tcfg = R.default_config(**SKULL_KW), R.default_config(**TUMOR_KW)
        Ps = S.randomised_params(scfg, S.padded(shape, 4), SEED + 10)
        Pt = S.randomised_params(tcfg, S.padded(shape, 8), SEED + 20)
        skull = engine_stage(SKULL_KW, Ps, S.padded(shape, 4), SKULL_STATS, 4)
        tumor = engine_stage(TUMOR_KW, Pt, S.padded(shape, 8), TUMOR_STATS, 8)
        y, lab, st = infer.segment_case(tumor, x, pixdim, skull=skull, return_stages=True)
        torch.cuda.synchronize()
        out[pixdim] = dict(x=x, shape=shape, scfg=scfg, tcfg=tcfg, Ps=Ps, Pt=Pt, skull=skull, tumor=tumor, y=y, lab=lab,
                           st={k: v.cpu().numpy() for k, v in st.items()})
    return out


@pytest.mark.parametrize('pixdim', [(1.2, 1.0, 0.9), (1.0, 1.0, 1.0)])
def test_two_stage_matches_the_oracle_stage_by_stage(two_stage, pixdim):
    """every stage against the oracle applied to the ENGINE's previous-stage output, so errors do not compound: probabilities of a TTA
    stage to 1e-4 absolute (the bound of tests/test_infer_gpu.py), the hand-over bit for bit, labels equal outside the ambiguous set"""
    r = two_stage[pixdim]
    st, shape = r['st'], r['shape']
    d, h, w = shape
    assert shape == ((13, 9, 13) if pixdim[0] != 1.0 else VOL)
    assert st['x1mm'].shape == S.padded(shape, 4) + (2,) and st['mask'].shape == S.padded(shape, 4) + (1,)
    assert st['x_stripped'].shape == S.padded(shape, 8) + (2,) and st['mask_repadded'].shape == S.padded(shape, 8) + (1,)
    assert 0.0 < st['mask'][:d, :h, :w].mean() < 1.0
    # skull stage
    p_ref = S.stage_prob(st['x1mm'], st['mask'], r['Ps'], r['scfg'], *SKULL_STATS)
    assert st['skull_prob'].shape == p_ref.shape == S.padded(shape, 4) + (1,)
    err = float(np.abs(st['skull_prob'] - p_ref).max())
    print('skull probability: max abs err %.3e (range %.3f..%.3f)' % (err, p_ref.min(), p_ref.max()))
    assert err <= 1e-4
    assert p_ref.max() - p_ref[st['mask'] > 0].min() > 0.1          # the stage does something: the strip is not a constant factor
    # hand-over: bit-equal to the numpy expression on the engine's own skull_prob
    xo_ref, mo_ref = S.strip(st['x1mm'], st['skull_prob'], st['mask'], shape, S.padded(shape, 8))
    assert np.array_equal(st['x_stripped'].view(np.uint32), xo_ref.view(np.uint32))
    assert np.array_equal(st['mask_repadded'].view(np.uint32), mo_ref.view(np.uint32))
    # tumour stage
    y_ref = S.stage_prob(st['x_stripped'], st['mask_repadded'], r['Pt'], r['tcfg'], *TUMOR_STATS)[:d, :h, :w]
    assert st['prob_1mm'].shape == y_ref.shape == shape + (3,)
    err = float(np.abs(st['prob_1mm'] - y_ref).max())
    print('tumour probability: max abs err %.3e' % err)
    assert err <= 1e-4
    # way back and labels
    prob, mback = S.reverse(st['prob_1mm'], st['mask'][:d, :h, :w], VOL, pixdim, 3)
    lab_ref = S.labels(prob, mback, 0.5)
    amb = S.ambiguous(prob, 0.5, 1e-4)
    lab = r['lab'].cpu().numpy()
    assert lab.shape == VOL and lab.dtype == np.uint8 and tuple(r['y'].shape) == VOL + (3,)
    print('labels: %d of %d ambiguous, %d differ' % (int(amb.sum()), amb.size, int((lab != lab_ref).sum())))
    assert amb.mean() <= 0.01
    assert int(((lab != lab_ref) & ~amb).sum()) == 0
    assert set(np.unique(lab).tolist()) <= {0, 1, 2, 4} and len(np.unique(lab)) >= 3
    assert float(np.abs(r['y'].cpu().numpy() - prob).max()) <= 1e-4


@pytest.mark.parametrize('pixdim', [(1.2, 1.0, 0.9), (1.0, 1.0, 1.0)])
def test_segment_case_without_skull_is_segment_scan(two_stage, pixdim):
    from bts_amd import infer
    r = two_stage[pixdim]
    t = r['tumor']
    y0, lab0 = infer.segment_scan(t.model, r['x'], pixdim, t.mean, t.std, 8)
    y1, lab1, st = infer.segment_case(t, r['x'], pixdim, return_stages=True)
    y2, lab2 = infer.segment_case(t, torch.from_numpy(r['x']).to(dev()), pixdim)
    assert torch.equal(y0, y1) and torch.equal(lab0, lab1) and torch.equal(y0, y2) and torch.equal(lab0, lab2)
    assert st['skull_prob'] is None and st['x_stripped'] is None and st['mask_repadded'] is None
    assert tuple(st['x1mm'].shape) == S.padded(r['shape'], 8) + (2,) and tuple(st['prob_1mm'].shape) == r['shape'] + (3,)
    assert not torch.equal(lab0, r['lab'])                           # ... and the skull stage changes the answer


def test_skull_model_must_have_one_output_channel(two_stage):
    from bts_amd import infer
    from bts_amd.model import Model
    r = two_stage[(1.0, 1.0, 1.0)]
    m = Model(**dict(SKULL_KW, out_ch=3))
    m.build((1,) + S.padded(VOL, 4) + (2,))
    bad = infer.StageSpec(m, r['skull'].mean, r['skull'].std, 4)
    with pytest.raises(ValueError, match='out_ch == 1.*out_ch = 3'):
        infer.segment_case(r['tumor'], r['x'], (1.0, 1.0, 1.0), skull=bad)


# ---- the command -------------------------------------------------------------------------------------------------------------------
def write_case(folder, vol, seed, affine, seg):
    from bts_amd import nifti
    os.makedirs(folder)
    x = S.scan_like(vol, seed)
    nifti.save(os.path.join(folder, 'c_t1ce.nii.gz'), x[..., 0], affine)
    nifti.save(os.path.join(folder, 'c_flair.nii'), x[..., 1], affine)
    if seg:
        y = np.array([0, 1, 2, 4], dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=vol)]
        nifti.save(os.path.join(folder, 'c_seg.nii.gz'), y.astype(np.int16), affine)
        return y
    return None


def write_model(folder, kw, build, crop_size, seed):
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    cfg = R.default_config(**kw)
    m = Model(**kw)
    m.build((1,) + tuple(build) + (2,))
    m.set_weights_from(S.randomised_params(cfg, tuple(build), seed))
    save_checkpoint(folder, m)
    args = {'model_args': dict(kw)}
    if crop_size:
        args['crop_size'] = list(build)
    save_train_args(folder, args)


def test_command_end_to_end(tmp_path, capsys):
    """three cases (two modalities; one with non-unit pixdim, one unlabelled), two checkpoints (the tumour model's train_args.pkl
    records a crop size that is NOT the cases' padded extent, the skull model's records none), --workers 0 against --workers 2"""
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti
    from bts_amd import test as T
    data = tmp_path / 'data'
    truth = {'a': write_case(str(data / 'a'), VOL, 5, np.eye(4), True),
             'b': write_case(str(data / 'b'), VOL, 6, np.diag([1.2, 1.0, 0.9, 1.0]), True),
             'c': write_case(str(data / 'c'), VOL, 7, np.eye(4), False)}
    write_model(str(tmp_path / 'tumor'), TUMOR_KW, (32, 16, 16), True, SEED + 20)
    write_model(str(tmp_path / 'skull'), SKULL_KW, S.padded(VOL, 4), False, SEED + 10)
    for name, (mean, std) in (('tp.npy', TUMOR_STATS), ('sp.npy', SKULL_STATS)):
        np.save(str(tmp_path / name), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                       'norm': {'mean': np.array(mean).reshape(1, 1, 1, 2), 'std': np.array(std).reshape(1, 1, 1, 2)}})
    outs = []
    for workers in (0, 2):
        out = tmp_path / ('out%d' % workers)
        assert T.main(['--in_locs', str(data), '--modalities', 't1ce,flair', '--truth', 'seg', '--gpu',
                       '--tumor_model', str(tmp_path / 'tumor'), '--tumor_prepro', str(tmp_path / 'tp.npy'),
                       '--skull_model', str(tmp_path / 'skull'), '--skull_prepro', str(tmp_path / 'sp.npy'),
                       '--workers', str(workers), '--out_loc', str(out)]) == 0
        outs.append(out)
    text = capsys.readouterr().out
    assert text.count('3 cases segmented (2 scored)') == 2 and text.count('a. Macro: ') == 2 and 'c. Macro' not in text
    conf = np.zeros((4, 4), dtype=np.int64)
    masks = {}
    for case in ('a', 'b', 'c'):
        b0, b1 = (open(str(o / case / 'mask.nii'), 'rb').read() for o in outs)
        assert b0 == b1, case
        lab, hdr = nifti.load(str(outs[0] / case / 'mask.nii'))
        assert lab.shape == VOL and lab.dtype == np.uint8 and set(np.unique(lab).tolist()) <= {0, 1, 2, 4}
        masks[case] = lab
    assert np.allclose(nifti.load(str(outs[0] / 'b' / 'mask.nii'))[1]['pixdim'][1:4], [1.2, 1.0, 0.9])
    assert len(set(m.tobytes() for m in masks.values())) == 3 and all(m.any() for m in masks.values())
    csv0, csv1 = (open(str(o / 'scores.csv')).read() for o in outs)
    assert csv0 == csv1
    rows = [r.split(',') for r in csv0.strip().split('\n')]
    assert [r[0] for r in rows] == ['case', 'a', 'b', 'total'] and all(len(r) == 9 for r in rows)
    for row, case in ((rows[1], 'a'), (rows[2], 'b')):
        s = infer.label_scores(truth[case], masks[case])
        assert row == T.score_row(case, s)
        conf += s['confusion']
    assert int(conf.sum()) == 2 * VOL[0] * VOL[1] * VOL[2]
    assert rows[3] == T.score_row('total', infer.scores_from_confusion(conf))
