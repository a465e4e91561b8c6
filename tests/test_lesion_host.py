"""CPU: the SciPy restatement of the lesion-wise score (tests/lesion_ref.py) against hand-made maps with known answers, the argument
validation of the entry points of csrc/lesion.hip, and the --lesionwise flags and columns of `python -m bts_amd.test`.  No kernel runs
here; the device side is tests/test_lesion_gpu.py."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lesion_ref as L  # noqa: E402

import bts_amd  # noqa: E402,F401
from bts_amd import test as T  # noqa: E402

REQUIRED = ['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--tumor_prepro', 'p.npy', '--tumor_model', 'm']
UNIT = (1.0, 1.0, 1.0)
ZERO = L.ZERO


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize('name', sorted(L.known_cases()))
def test_the_restatement_gives_the_known_answers(name):
    t, p, kw, (dice, hd, counts) = L.known_cases()[name]
    got = L.lesionwise_region(t, p, UNIT, **kw)
    assert same(got[0], dice) and got[2] == counts, (name, got)
    if hd is not None:
        assert same(got[1], hd), (name, got)
    assert len(got[3]) == counts['lesions']


def test_halo_only_match_is_scored_not_penalised():
    t, p, kw, _ = L.known_cases()['halo_only']
    dice, hd, counts, rows = L.lesionwise_region(t, p, UNIT, **kw)
    assert rows == [dict(voxels=64, matched_components=1, matched_voxels=64, overlap=0, dice=0.0, hd95=rows[0]['hd95'])]
    assert counts['false_positives'] == 0 and counts['false_negatives'] == 0
    assert math.isfinite(hd) and 2.0 < hd < 374.0 and hd == rows[0]['hd95']          # surfaces 3 .. 9 voxels apart along W
    # one voxel further and the component is outside the halo: a missed lesion and a false positive
    p2 = np.roll(p, 2, axis=2)
    dice, hd, counts, rows = L.lesionwise_region(t, p2, UNIT)
    assert (dice, hd) == (0.0, 374.0) and counts == dict(ZERO, lesions=1, false_negatives=1, false_positives=1)


def test_one_component_spanning_two_lesions_counts_for_both():
    t, p, kw, _ = L.known_cases()['one_component_two_lesions']
    dice, hd, counts, rows = L.lesionwise_region(t, p, UNIT)
    assert [r['matched_components'] for r in rows] == [1, 1] and [r['matched_voxels'] for r in rows] == [64, 64]
    assert [r['overlap'] for r in rows] == [16, 16] and counts['false_positives'] == 0
    assert hd == (rows[0]['hd95'] + rows[1]['hd95']) / 2


def test_scores_dict_and_the_order_of_lesions():
    t, p = L.multi_lesion_pair()
    r = L.lesionwise_scores(t, p, (1.2, 1.0, 0.9))
    assert set(r) == {'lw_%s_%s' % (a, b) for a in ('dice', 'hd95', 'counts', 'lesions') for b in ('wt', 'tc', 'et')}
    assert r['lw_counts_wt'] == {'lesions': 5, 'false_negatives': 1, 'false_positives': 1, 'ignored': 1}
    assert [x['voxels'] for x in r['lw_lesions_wt']] == [360, 384, 384, 192, 180]      # by the first voxel of the dilated component
    assert [x['matched_components'] for x in r['lw_lesions_wt']] == [1, 1, 1, 1, 0]
    assert r['lw_lesions_wt'][1]['overlap'] == 0 and r['lw_lesions_wt'][1]['hd95'] < 374.0           # through the halo only
    assert r['lw_lesions_wt'][2]['matched_voxels'] == r['lw_lesions_wt'][3]['matched_voxels'] == 224  # one component, two lesions
    assert r['lw_counts_et'] == {'lesions': 2, 'false_negatives': 0, 'false_positives': 1, 'ignored': 2}
    n = 6
    assert r['lw_dice_wt'] == sum(x['dice'] for x in r['lw_lesions_wt']) / n
    assert r['lw_hd95_wt'] == (sum(x['hd95'] for x in r['lw_lesions_wt']) + 374.0) / n
    two = L.lesionwise_scores(np.minimum(t, 1), np.minimum(p, 1), (1.2, 1.0, 0.9), n_classes=2)
    assert set(two) == {'lw_dice_class_1', 'lw_hd95_class_1', 'lw_counts_class_1', 'lw_lesions_class_1'}
    assert two['lw_lesions_class_1'] == r['lw_lesions_wt']


def test_pieces_of_the_restatement_on_a_known_map():
    t, p = np.zeros((2, 3, 8), bool), np.zeros((2, 3, 8), bool)
    t[0, 0, 0:2] = True                                  # lesion of root 0
    t[1, 2, 6:8] = True                                  # lesion whose dilated component starts at (0,2,6): root 22
    p[0, 0, 1:4] = True                                  # component of root 1: one voxel on the first lesion, one in its halo
    p[1, 1, 7] = True                                    # component of root 39: in the second lesion's halo only
    td = L.components(L.dilate(t, 6, 1), 26)
    pc = L.components(p, 26)
    assert L.roots_of(td).tolist() == [0, 22] and L.roots_of(pc).tolist() == [1, 39]
    rows, vox = L.pairs(td, t, pc)
    assert rows.tolist() == [[0, 1, 2, 1], [22, 39, 1, 0]] and vox[0] == 2 and vox[22] == 2 and int(vox.sum()) == 4
    assert L.boxes(pc, [1, 39]).tolist() == [[0, 0, 1, 1, 1, 4], [1, 1, 7, 2, 2, 8]]
    g, m = L.crop(td, t, pc, (0, 0, 0, 1, 2, 4), 0, [1])
    assert g.tolist() == [[[1, 1, 0, 0], [0, 0, 0, 0]]] and m.tolist() == [[[0, 1, 1, 1], [0, 0, 0, 0]]]


def test_entry_points_validate_before_any_hip_call():
    """BTS_ERR_SHAPE (-1) with NULL pointers and no GPU"""
    from bts_amd._lib import lib
    lb = lib()
    big = 2 ** 31 - 1

    def dil(d=4, h=5, w=6, k=4, cm=14, conn=18, it=3, fuse=0):
        return lb._bts_dilate3d(None, None, d, h, w, k, cm, conn, it, fuse, None, None)

    for name in ('d', 'h', 'w'):
        assert dil(**{name: 0}) == -1 and dil(**{name: -2}) == -1, name
    assert dil(d=1 << 11, h=1 << 10, w=1 << 10) == -1 and dil(d=46341, h=46341, w=46341) == -1
    for k in (-1, 0, 1, 9):
        assert dil(k=k) == -1, k
    assert dil(cm=-1) == -1 and dil(cm=16) == -1 and dil(k=2, cm=4) == -1
    for conn in (0, 4, 7, 8, 27):
        assert dil(conn=conn) == -1, conn
    assert dil(it=-1) == -1 and dil(it=4097) == -1 and dil(fuse=-1) == -1 and dil(fuse=7) == -1
    assert dil(it=4, fuse=2) == -4                                                  # two passes and no workspace: BTS_ERR_WORKSPACE
    assert lb._bts_dilate3d_workspace(4, 5, 6, 3, 0) == 0 and lb._bts_dilate3d_workspace(4, 5, 6, 3, 1) == 120
    assert lb._bts_dilate3d_workspace(4, 5, 6, 0, 0) == 0 and lb._bts_dilate3d_workspace(4, 5, 6, 7, 0) == 120
    assert lb._bts_dilate3d_workspace(0, 5, 6, 3, 0) == -1 and lb._bts_dilate3d_workspace(4, 5, 6, -1, 0) == -1

    def pairs(n=10, k=4, cm=14, cap=16):
        return lb._bts_lesion_pairs(None, None, None, n, k, cm, None, None, cap, None, None)

    assert pairs(n=-1) == -1 and pairs(n=big) == -1 and pairs(k=1) == -1 and pairs(k=9) == -1 and pairs(cm=16) == -1 and pairs(cm=-1) == -1
    assert pairs(cap=0) == -1 and pairs(cap=-4) == -1 and pairs(cap=(1 << 32) + 1) == -1
    assert lb._bts_lesion_pairs_table_bytes(0) == -1 and lb._bts_lesion_pairs_table_bytes(1) == 16
    assert lb._bts_lesion_pairs_table_bytes(1 << 20) == 16 << 20

    def boxes(d=4, h=5, w=6, m=3):
        return lb._bts_component_boxes(None, d, h, w, None, m, None, None)

    assert boxes(d=0) == -1 and boxes(h=-1) == -1 and boxes(w=0) == -1 and boxes(m=-1) == -1 and boxes(d=1 << 11, h=1 << 10, w=1 << 10) == -1
    assert boxes(m=0) == 0                                                          # nothing to do, nothing launched

    def crop(d=4, h=5, w=6, k=4, cm=14, box=(0, 0, 0, 4, 5, 6), root=0, m=0):
        return lb._bts_lesion_crop(None, None, None, d, h, w, k, cm, *box, root, None, m, None, None, None)

    assert crop(d=0) == -1 and crop(k=1) == -1 and crop(cm=16) == -1 and crop(m=-1) == -1
    for box in ((-1, 0, 0, 4, 5, 6), (0, 0, 0, 5, 5, 6), (0, 0, 0, 4, 6, 6), (0, 0, 0, 4, 5, 7), (2, 0, 0, 2, 5, 6), (0, 3, 0, 4, 2, 6),
                (0, 0, 6, 4, 5, 6)):
        assert crop(box=box) == -1, box
    assert crop(root=-1) == -1 and crop(root=120) == -1


def test_the_flags_parse_default_to_off_and_refuse_nonsense(capsys):
    args = T.parse_args(REQUIRED)
    assert T.lesion_kwargs(args) is None
    assert T.lesion_kwargs(T.parse_args(REQUIRED + ['--lesionwise'])) == {'dilation': 3, 'min_lesion_voxels': 50, 'penalty_mm': 374.0}
    got = T.parse_args(REQUIRED + ['--lesionwise', '--lesion_dilation', '0', '--lesion_min_voxels', '7', '--lesion_penalty_mm', '100.5'])
    assert T.lesion_kwargs(got) == {'dilation': 0, 'min_lesion_voxels': 7, 'penalty_mm': 100.5}
    assert T.lesion_kwargs(T.parse_args(REQUIRED + ['--lesion_dilation', '2'])) is None            # a parameter alone asks for nothing
    for bad in (['--lesion_dilation', '-1'], ['--lesion_min_voxels', '-5'], ['--lesion_penalty_mm', '-0.5'], ['--lesion_penalty_mm', 'nan'],
                ['--lesion_dilation', '1.5'], ['--lesionwise', '1']):
        with pytest.raises(SystemExit):
            T.parse_args(REQUIRED + bad)
    capsys.readouterr()


def test_the_plain_command_line_parses_as_before():
    """without the new flags the namespace is the one the command had: no new attribute, nothing changed"""
    before = vars(T.parse_args(REQUIRED))
    assert not any(k.startswith('lesion') for k in before)
    after = vars(T.parse_args(REQUIRED + ['--lesionwise']))
    assert set(after) - set(before) == {'lesionwise'} and all(after[k] == v for k, v in before.items())


def test_column_layout():
    assert T.LESION_KEYS == ('lw_dice_wt', 'lw_dice_tc', 'lw_dice_et', 'lw_hd95_wt', 'lw_hd95_tc', 'lw_hd95_et',
                             'lw_lesions_wt', 'lw_lesions_tc', 'lw_lesions_et', 'lw_fn_wt', 'lw_fn_tc', 'lw_fn_et',
                             'lw_fp_wt', 'lw_fp_tc', 'lw_fp_et')
    t, p = L.multi_lesion_pair()
    cols = T.lesion_columns(L.lesionwise_scores(t, p, (1.2, 1.0, 0.9)))
    assert set(cols) == set(T.LESION_KEYS)
    row = T.lesion_row(cols)
    assert len(row) == 15 and row[0] == '%.6f' % cols['lw_dice_wt'] and row[5] == '%.6f' % cols['lw_hd95_et']
    assert row[6:] == ['5', '4', '2', '1', '1', '0', '1', '1', '1']
    nan = dict(cols, lw_dice_wt=float('nan'))
    assert T.lesion_row(nan)[0] == 'nan'
