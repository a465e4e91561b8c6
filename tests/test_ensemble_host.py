"""Without a GPU: the host side of ensembles and uncertainty maps -- the reduction of the (level, pair) table to the uncertainty-filtered
scores against hand cases and the brute force of tests/ensemble_ref.py, what `infer.StageEnsemble` refuses, and the command line's
--tumor_model A,B,C, --tumor_prepro and --uncertainty."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ensemble_ref as E  # noqa: E402

import bts_amd  # noqa: E402,F401
from bts_amd import infer  # noqa: E402
from bts_amd import test as T  # noqa: E402

REQUIRED = ['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--tumor_model', 'm', '--tumor_prepro', 'p.npy']


# ---- the reduction ---------------------------------------------------------------------------------------------------------------
def test_perfect_prediction_with_level_zero_scores_one():
    counts = np.zeros((101, 4), dtype=np.int64)
    counts[0] = [900, 0, 0, 100]                                        # every voxel right, every voxel certain
    assert infer.uncertainty_scores_from_counts(counts) == (1.0, 1.0, 0.0, 0.0)


def test_errors_at_level_100_and_correct_voxels_at_level_0():
    """Dice(tau) is 1 up to tau = 99, where no error is kept, and the plain Dice at tau = 100: 99 intervals of the trapezoid hold 1 and
    the last (1 + Dice_100) / 2; nothing correct is ever filtered out"""
    tn, fp, fn, tp = 700, 30, 50, 220
    counts = np.zeros((101, 4), dtype=np.int64)
    counts[0] = [tn, 0, 0, tp]
    counts[100] = [0, fp, fn, 0]
    dice100 = 2.0 * tp / (2.0 * tp + fp + fn)
    score, a_dice, a_ftp, a_ftn = infer.uncertainty_scores_from_counts(counts)
    assert a_dice == pytest.approx((99.0 + (dice100 + 1.0) / 2.0) / 100.0, rel=1e-15)
    assert a_ftp == 0.0 and a_ftn == 0.0
    assert score == pytest.approx((a_dice + 2.0) / 3.0, rel=1e-15)


def test_empty_denominators():
    """no voxel at all: Dice 1 at every threshold, nothing to filter; no true positive: FTP 0, not nan"""
    assert infer.uncertainty_scores_from_counts(np.zeros((101, 4), dtype=np.int64)) == (1.0, 1.0, 0.0, 0.0)
    counts = np.zeros((101, 4), dtype=np.int64)
    counts[40] = [10, 5, 0, 0]
    score, a_dice, a_ftp, a_ftn = infer.uncertainty_scores_from_counts(counts)
    assert a_ftp == 0.0 and 0.0 < a_ftn < 1.0 and np.isfinite(score)
    assert a_dice == pytest.approx(39.5 / 100.0) and a_ftn == pytest.approx(39.5 / 100.0)   # 1 up to 39, (1 + 0) / 2 across 39..40, then 0
    with pytest.raises(ValueError, match=r'\(101, 4\)'):
        infer.uncertainty_scores_from_counts(np.zeros((100, 4)))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reduction_equals_the_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = 4000
    t = np.array([0, 0, 1, 2, 4], dtype=np.uint8)[rng.integers(0, 5, size=n)]
    p = np.where(rng.random(n) < 0.7, t, np.array([0, 1, 2, 4], dtype=np.uint8)[rng.integers(0, 4, size=n)]).astype(np.uint8)
    u = np.where((t != p)[:, None], rng.integers(30, 101, size=(n, 3)), rng.integers(0, 60, size=(n, 3))).astype(np.uint8)
    m = (rng.random(n) > 0.2).astype(np.uint8)
    for targets in ('labels', 'regions'):
        table = E.table(t, p, u, E.class_masks(targets), m)
        for counts in table:
            got, ref = infer.uncertainty_scores_from_counts(counts), E.scores(counts)
            assert got == pytest.approx(ref, rel=1e-13, abs=1e-15)
            assert 0.0 < got[1] <= 1.0 and 0.0 <= got[2] < 1.0 and 0.0 <= got[3] < 1.0


def test_channel_names():
    assert [n for n, _ in infer.uncertainty_channels('regions')] == ['wt', 'tc', 'et']
    assert infer.uncertainty_channels('regions') == infer.BRATS_REGIONS
    assert infer.uncertainty_channels('labels') == (('class_1', (1,)), ('class_2', (2,)), ('class_3', (3,)))
    with pytest.raises(ValueError):
        infer.uncertainty_channels('classes')
    assert T.uncertainty_keys('regions')[:4] == ('qu_score_wt', 'qu_score_tc', 'qu_score_et', 'qu_dice_auc_wt')
    assert len(T.uncertainty_keys('labels')) == len(T.uncertainty_keys('regions')) == 12


def test_scores_refuse_label_maps_of_another_type():
    t = torch.zeros((4, 5, 6), dtype=torch.uint8)
    with pytest.raises(ValueError, match='label maps must be uint8'):
        infer.uncertainty_scores(t.numpy().astype(np.int16), t.numpy(), np.zeros((4, 5, 6, 3), np.uint8))


# ---- StageEnsemble ---------------------------------------------------------------------------------------------------------------
class StubDecoder(object):
    def __init__(self, out_ch):
        self.out_ch = out_ch


class StubModel(object):
    def __init__(self, out_ch=3):
        self.decoder = StubDecoder(out_ch)


def stage(out_ch=3, res=8, **kw):
    return infer.StageSpec(StubModel(out_ch), np.zeros(2), np.ones(2), res, **kw)


def test_ensemble_exposes_what_segment_case_reads():
    a, b = stage(), stage(spatial_tta=False)
    ens = infer.StageEnsemble([a, b], 'std')
    assert (ens.spatial_res, ens.data_format, ens.threshold, ens.targets, ens.out_ch) == (8, 'channels_last', 0.5, 'labels', 3)
    assert ens.members == [a, b] and ens.uncertainty == 'std' and ens.window_counts is None
    assert infer.StageEnsemble([a]).uncertainty is None and infer.StageEnsemble((a,), 'entropy').uncertainty == 'entropy'
    tta = ens.augmentor()
    assert isinstance(tta, infer.EnsembleAugmentor) and tta.threshold == 0.5 and tta.targets == 'labels'
    with pytest.raises(ValueError, match='multiple of the model'):
        ens.augmentor(infer.WindowSpec((12, 8, 8)))


@pytest.mark.parametrize('other,what', [
    (dict(res=4), r'member 1 has spatial_res = 4, member 0 has 8'),
    (dict(out_ch=4), r'member 1 has out_ch = 4, member 0 has 3'),
    (dict(targets='regions'), r"member 1 has targets = 'regions', member 0 has 'labels'"),
    (dict(threshold=0.4), r'member 1 has threshold = 0.4, member 0 has 0.5'),
    (dict(compute_dtype='float16'), r"member 1 has compute_dtype = 'float16', member 0 has 'float32'"),
])
def test_ensemble_refuses_members_that_differ(other, what):
    with pytest.raises(ValueError, match=what):
        infer.StageEnsemble([stage(), stage(**other)])
    infer.StageEnsemble([stage(**other), stage(**other)])                # ... and takes them when they agree


def test_ensemble_refuses_the_rest():
    with pytest.raises(ValueError, match='non-empty list of StageSpec'):
        infer.StageEnsemble([])
    with pytest.raises(ValueError, match='non-empty list of StageSpec'):
        infer.StageEnsemble([stage(), StubModel()])
    with pytest.raises(ValueError, match="'std' is the spread between members and needs two at least, got 1"):
        infer.StageEnsemble([stage()], 'std')
    with pytest.raises(ValueError, match="got 'variance'"):
        infer.StageEnsemble([stage(), stage()], 'variance')


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_a_plain_command_line_parses_to_what_it_did():
    args = vars(T.parse_args(REQUIRED))
    assert args == {'in_locs': ['a', 'b'], 'modalities': ['t1ce', 'flair'], 'truth': '', 'tumor_prepro': 'p.npy', 'skull_prepro': '',
                    'tumor_model': 'm', 'skull_model': '', 'order': 3, 'mode': 'reflect', 'spatial_tta': True, 'channel_tta': 0,
                    'threshold': 0.5, 'gpu': False, 'dtype': 'float32', 'tta_batch': None, 'workers': 8, 'out_loc': '',
                    'surface_metrics': False, 'skull_strip': False, 'min_component_voxels': 0, 'et_min_voxels': 0,
                    'component_connectivity': 26, 'skull_largest_component': False}
    ns = T.parse_args(REQUIRED)
    assert T.tumor_models(ns) == ['m'] and T.tumor_prepros(ns) == ['p.npy']


def line(models, prepros, *more):
    return ['--in_locs', 'a', '--modalities', 't1ce', '--tumor_model', models, '--tumor_prepro', prepros] + list(more)


def test_comma_lists():
    args = T.parse_args(line('A,B,C', 'p.npy'))
    assert args.tumor_model == 'A,B,C' and args.tumor_prepro == 'p.npy' and not hasattr(args, 'uncertainty')      # the strings they were
    assert T.tumor_models(args) == ['A', 'B', 'C'] and T.tumor_prepros(args) == ['p.npy'] * 3
    args = T.parse_args(line('A,B,C', 'a.npy,b.npy,c.npy', '--uncertainty', 'std'))
    assert T.tumor_prepros(args) == ['a.npy', 'b.npy', 'c.npy'] and args.uncertainty == 'std'
    assert T.parse_args(line('A', 'p.npy', '--uncertainty', 'entropy')).uncertainty == 'entropy'
    assert T.parse_args(line('A,B', 'p.npy', '--uncertainty', 'entropy')).uncertainty == 'entropy'


@pytest.mark.parametrize('argv,message', [
    (line('A,B,C', 'a.npy,b.npy'), '2 files for 3 models'),
    (line('A', 'a.npy,b.npy'), '2 files for 1 models'),
    (line('A', 'p.npy', '--uncertainty', 'std'), 'needs two at least'),
    (line('A,B', 'p.npy', '--uncertainty', 'variance'), 'invalid choice'),
    (line(',', 'p.npy'), 'names no checkpoint folder'),
])
def test_parse_time_errors(argv, message, capsys):
    with pytest.raises(SystemExit) as info:
        T.parse_args(argv)
    assert info.value.code == 2 and message in capsys.readouterr().err
