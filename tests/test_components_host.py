"""CPU: the NumPy restatement of the connected-component post-processing (tests/components_ref.py) against SciPy and against hand-made
maps with known answers, the argument validation of the entry points of csrc/components.hip, and the new flags of `python -m
bts_amd.test`.  No kernel runs here; the device side is tests/test_components_gpu.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import components_ref as C  # noqa: E402

import bts_amd  # noqa: E402,F401
from bts_amd import test as T  # noqa: E402

SHAPES = [(5, 6, 7), (1, 9, 70), (17, 3, 300), (33, 70, 65), (9, 9, 65)]
REQUIRED = ['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--tumor_prepro', 'p.npy', '--tumor_model', 'm']


def canonical_scipy(region, c):
    ndi = pytest.importorskip('scipy.ndimage')
    labels, n = ndi.label(region, ndi.generate_binary_structure(3, c))
    out = np.zeros(region.shape, dtype=np.int32)
    if n:
        ids = np.arange(1, n + 1)
        first = ndi.minimum(np.arange(region.size).reshape(region.shape), labels, ids) + 1
        out = np.concatenate([[0], first])[labels].astype(np.int32)
    return out


@pytest.mark.parametrize('c,connectivity', [(1, 6), (2, 18), (3, 26)])
@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_against_scipy(shape, c, connectivity):
    maps = [C.random_labels(shape, 0.5, 1), C.random_labels(shape, 0.05, 2), C.checkerboard(shape), C.serpentine(shape),
            np.ones(shape, np.uint8), np.zeros(shape, np.uint8)]
    for i, lab in enumerate(maps):
        for cm, k in ((14, 4), (8, 4), (1, 4), (2, 2)):
            region = C.region_of(lab, cm, k)
            got = C.components3d(lab, cm, k, connectivity)
            assert got.dtype == np.int32 and np.array_equal(got, canonical_scipy(region, c)), (i, cm, k)


def test_connectivities_differ_where_they_should():
    board = C.checkerboard((4, 5, 6))
    assert C.sizes(C.components3d(board, 2, 2, 6))[1] == int(board.sum())          # all singletons by faces
    assert C.sizes(C.components3d(board, 2, 2, 18))[1] == 1                        # ... one component by edges
    edge = np.zeros((3, 3, 3), np.uint8)
    edge[0, 0, 0] = edge[0, 1, 1] = 1
    corner = np.zeros((3, 3, 3), np.uint8)
    corner[0, 0, 0] = corner[1, 1, 1] = 1
    assert [C.sizes(C.components3d(edge, 2, 2, c))[1] for c in (6, 18, 26)] == [2, 1, 1]
    assert [C.sizes(C.components3d(corner, 2, 2, c))[1] for c in (6, 18, 26)] == [2, 2, 1]
    assert C.sizes(C.components3d(C.serpentine((7, 9, 5)), 2, 2, 6))[1] == 1


def test_largest_and_its_tie_rule_on_a_known_map():
    """two components of 3 voxels (roots 2 and 20) and one of 2 (root 12): the lower root of the equal pair is kept"""
    lab = np.zeros((2, 3, 5), np.uint8)
    lab[0, 0, 2:5] = 1                 # indices 2, 3, 4
    lab[0, 2, 2:4] = 2                 # indices 12, 13
    lab[1, 1, 0:3] = 4                 # indices 20, 21, 22
    comp = C.components3d(lab, 14, 4, 6)
    assert sorted(set(comp.reshape(-1).tolist())) == [0, 3, 13, 21]
    size, found = C.sizes(comp)
    assert found == 3 and size[2] == 3 and size[12] == 2 and size[20] == 3 and int(size.sum()) == 8
    key = C.largest_key(size)
    assert key == (3 << 32) | (0xFFFFFFFF - 2) and C.key_root(key) == 2
    out, vox, gone = C.apply(lab, comp, size, largest_only=True)
    assert (vox, gone) == (5, 2)
    want = np.zeros_like(lab)
    want[0, 0, 2:5] = 1
    assert np.array_equal(out, want)
    assert C.largest_key(np.zeros(7, np.int32)) == 0
    # by size: the pair of 2 goes at min_voxels 3, nothing at 2; `fill` is what is written
    out, vox, gone = C.apply(lab, comp, size, min_voxels=3, fill=9)
    assert (vox, gone) == (2, 1) and np.array_equal(out[0, 2, 2:4], [9, 9]) and int((out != lab).sum()) == 2
    assert C.apply(lab, comp, size, min_voxels=2)[1:] == (0, 0)


def test_postprocess_labels_on_known_maps():
    lab = np.zeros((4, 6, 8), np.uint8)
    lab[0, 0, 0:4] = 2                 # a whole-tumour piece of 4 voxels: labels 2, 2, 1, 4 in one component
    lab[0, 0, 2] = 1
    lab[0, 0, 3] = 4
    lab[2, 3, 3:6] = 2                 # a speck of 3 voxels
    lab[3, 5, 7] = 4                   # a speck of 1: enhancing
    # (a) a speck of min - 1 voxels is removed, one of exactly min is kept
    out, c = C.postprocess_labels(lab, min_component_voxels=4)
    assert c == {'components': 3, 'removed_components': 2, 'removed_voxels': 4, 'et_relabelled': 0}
    assert np.array_equal(out[0, 0, 0:4], [2, 2, 1, 4]) and int(out.sum()) == 9 and out[2, 3, 4] == 0 and out[3, 5, 7] == 0
    out, c = C.postprocess_labels(lab, min_component_voxels=3)
    assert c['removed_components'] == 1 and c['removed_voxels'] == 1 and np.array_equal(out[2, 3, 3:6], [2, 2, 2])
    # (b) two enhancing voxels in all: relabelled at et_min_voxels 3 (one fewer), kept at 2 (exactly as many)
    out, c = C.postprocess_labels(lab, et_min_voxels=3)
    assert c['et_relabelled'] == 2 and out[0, 0, 3] == 1 and out[3, 5, 7] == 1 and not (out == 4).any()
    out, c = C.postprocess_labels(lab, et_min_voxels=2)
    assert c['et_relabelled'] == 0 and np.array_equal(out, lab)
    # (a) before (b): the stray enhancing voxel goes first, and the one that is left is then below 2
    out, c = C.postprocess_labels(lab, min_component_voxels=2, et_min_voxels=2)
    assert c == {'components': 3, 'removed_components': 1, 'removed_voxels': 1, 'et_relabelled': 1}
    assert out[3, 5, 7] == 0 and np.array_equal(out[0, 0, 0:4], [2, 2, 1, 1])
    # nothing asked, nothing done
    out, c = C.postprocess_labels(lab)
    assert np.array_equal(out, lab) and not any(c.values())


def test_entry_points_validate_before_any_hip_call():
    """BTS_ERR_SHAPE (-1) with NULL pointers and no GPU; nothing to do returns 0 without a launch"""
    from bts_amd._lib import lib
    L = lib()

    def label(d=4, h=5, w=6, k=4, cm=14, conn=26):
        return L._bts_components3d(None, None, d, h, w, k, cm, conn, None)

    for name in ('d', 'h', 'w'):
        assert label(**{name: 0}) == -1 and label(**{name: -3}) == -1, name
    assert label(d=1 << 11, h=1 << 10, w=1 << 10) == -1                             # 2^31 voxels
    assert label(d=2 ** 31 - 1, h=1, w=1) == -1 and label(d=1, h=2 ** 31 - 1, w=1) == -1 and label(d=1, h=1, w=2 ** 31 - 1) == -1
    assert label(d=46341, h=46341, w=46341) == -1                                   # the product leaves 64 bits of int arithmetic alone
    for k in (-1, 0, 1, 9, 64):
        assert label(k=k) == -1, k
    assert label(cm=-1) == -1 and label(cm=16) == -1 and label(k=2, cm=4) == -1
    for conn in (-6, 0, 4, 8, 7, 27):
        assert label(conn=conn) == -1, conn

    big = 2 ** 31 - 1
    assert L._bts_component_sizes(None, -1, None, None, None) == -1 and L._bts_component_sizes(None, big, None, None, None) == -1
    assert L._bts_component_sizes(None, 0, None, None, None) == 0
    assert L._bts_component_largest(None, -1, None, None) == -1 and L._bts_component_largest(None, big, None, None) == -1
    assert L._bts_component_largest(None, 0, None, None) == 0

    def apply(n=10, mv=0, lo=0, fill=0, key=None):
        return L._bts_components_apply(None, None, None, key, n, mv, lo, fill, None, None, None)

    assert apply(n=-1) == -1 and apply(n=big) == -1 and apply(mv=-1) == -1 and apply(fill=-1) == -1 and apply(fill=256) == -1
    assert apply(lo=1) == -1                                                        # largest_only without a key
    assert apply(n=0) == 0

    def relabel(n=10, k=4, cm=8, fill=1, limit=5):
        return L._bts_region_relabel(None, n, k, cm, fill, None, limit, None, None)

    assert relabel(n=-1) == -1 and relabel(k=1) == -1 and relabel(k=9) == -1 and relabel(cm=16) == -1 and relabel(cm=-1) == -1
    assert relabel(fill=256) == -1 and relabel(limit=-1) == -1
    assert relabel(n=0) == 0 and relabel(limit=0) == 0


def test_the_flags_parse_default_to_off_and_refuse_nonsense(capsys):
    args = T.parse_args(REQUIRED)
    assert (args.min_component_voxels, args.et_min_voxels, args.component_connectivity, args.skull_largest_component) == (0, 0, 26, False)
    assert T.postprocess_kwargs(args) is None
    got = T.parse_args(REQUIRED + ['--min_component_voxels', '50', '--et_min_voxels', '20', '--component_connectivity', '6'])
    assert T.postprocess_kwargs(got) == {'min_component_voxels': 50, 'et_min_voxels': 20, 'connectivity': 6}
    assert T.postprocess_kwargs(T.parse_args(REQUIRED + ['--et_min_voxels', '3'])) == \
        {'min_component_voxels': 0, 'et_min_voxels': 3, 'connectivity': 26}
    with_skull = REQUIRED + ['--skull_model', 's', '--skull_prepro', 's.npy']
    assert T.parse_args(with_skull + ['--skull_largest_component']).skull_largest_component is True
    assert T.parse_args(with_skull).skull_largest_component is False
    for bad in (['--skull_largest_component'], ['--min_component_voxels', '-1'], ['--et_min_voxels', '-5'],
                ['--component_connectivity', '8']):
        with pytest.raises(SystemExit):
            T.parse_args(REQUIRED + bad)
    capsys.readouterr()


def test_the_required_only_line_parses_as_before():
    """every attribute the command had before the post-processing flags, with the value it had"""
    args = vars(T.parse_args(REQUIRED))
    before = {'in_locs': ['a', 'b'], 'modalities': ['t1ce', 'flair'], 'truth': '', 'tumor_prepro': 'p.npy', 'skull_prepro': '',
              'tumor_model': 'm', 'skull_model': '', 'order': 3, 'mode': 'reflect', 'spatial_tta': True, 'channel_tta': 0,
              'threshold': 0.5, 'gpu': False, 'dtype': 'float32', 'tta_batch': None, 'workers': 8, 'out_loc': '',
              'surface_metrics': False, 'skull_strip': False}
    for k, v in before.items():
        assert args[k] == v, k
    assert set(args) - set(before) == {'min_component_voxels', 'et_min_voxels', 'component_connectivity', 'skull_largest_component'}
