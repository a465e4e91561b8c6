"""CPU: the restatement tests/labelvote_ref.py of the label vote (csrc/conform.hip: bts_label_resample3d) tied to the order-1 path of
tests/conform_ref.py, which tests/test_conform_host.py pins to SciPy; the inputs of tests/test_labelvote_gpu.py shown to hold no voxel
where the last bit of a weight decides, so that the GPU comparison needs no exclusion; and the host logic of
`python -m bts_amd.preprocess --conform`: the canvas, the truth's modality, the record and the flags."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import conform_ref  # noqa: E402
import labelvote_ref  # noqa: E402
from conform_ref import OUT, SRC, matrices  # noqa: E402

NAMES = ('oblique', 'anisotropic', 'permuting', 'integer')
INT_OUT = (37, 19, 23)
_CACHE = {}


def out_of(name):
    return INT_OUT if name == 'integer' else OUT


def voted(name):
    if name not in _CACHE:
        y = labelvote_ref.label_volume(SRC, 21)
        lab, margin = labelvote_ref.label_vote(y, matrices()[name], out_of(name))
        lab.setflags(write=False)
        _CACHE[name] = (y, lab, margin)
    return _CACHE[name]


def test_label_volume_is_what_it_says():
    y = labelvote_ref.label_volume(SRC, 21)
    assert y.dtype == np.float32 and set(np.unique(y).tolist()) == {0.0, 1.0, 2.0, 4.0}
    val, _ = labelvote_ref.taps(y, matrices()['oblique'], OUT)
    many = 1 + (np.diff(np.sort(val, axis=0), axis=0) != 0).sum(axis=0)
    print('distinct values among the 8 taps: %s' % {k: int((many == k).sum()) for k in range(1, 5)})
    assert (many >= 3).sum() >= 100 and (many == 4).sum() >= 1


@pytest.mark.parametrize('name', NAMES)
def test_vote_is_the_argmax_of_the_interpolated_indicators(name):
    y, lab, margin = voted(name)
    m, out = matrices()[name], out_of(name)
    values = np.array(labelvote_ref.VALUES)
    onehot = (y[..., None] == values.astype(np.float32)).astype(np.float64)
    p = conform_ref.interpolate(onehot, m, out, 1, np.float64)
    want = np.where(conform_ref.inside(m, out, SRC), values[np.argmax(p, axis=-1)], 0.0)
    sure = margin >= 1e-9
    assert sure.mean() > 0.99
    assert np.array_equal(lab[sure], want[sure].astype(np.float32))
    # the margin itself is the gap between the two largest interpolated indicators, to rounding
    top = np.sort(p, axis=-1)
    fov = conform_ref.inside(m, out, SRC)
    assert np.abs((top[..., -1] - top[..., -2])[fov] - margin[fov]).max() <= 1e-12


def test_integer_map_is_the_reorientation():
    y, lab, margin = voted('integer')
    assert np.array_equal(lab, conform_ref.reorient(y, (2, 0, 1), (False, True, False)))
    assert float(margin.min()) == 1.0                                   # all 8 taps on one voxel


@pytest.mark.parametrize('name', NAMES)
def test_two_values_is_thresholding_the_interpolated_indicator(name):
    y = (labelvote_ref.label_volume(SRC, 21) > 0).astype(np.float32)
    m, out = matrices()[name], out_of(name)
    lab, margin = labelvote_ref.label_vote(y, m, out)
    p = conform_ref.interpolate(y[..., None].astype(np.float64), m, out, 1, np.float64)[..., 0]
    sure = margin >= 1e-9
    assert np.array_equal(lab[sure], (p > 0.5).astype(np.float32)[sure])


@pytest.mark.parametrize('name', NAMES)
def test_the_gpu_cases_hold_no_voxel_where_the_last_bit_decides(name):
    """so tests/test_labelvote_gpu.py compares every voxel"""
    _, _, margin = voted(name)
    near = conform_ref.near_a_decision(matrices()[name], out_of(name), SRC, 1, eps=1e-6)
    print('%s: smallest margin %.3g, %d voxels near a face of the field of view' % (name, float(margin.min()), int(near.sum())))
    assert float(margin.min()) >= 1e-9
    assert not near.any()


@pytest.mark.parametrize('which', sorted(labelvote_ref.TIE_SHIFTS))
def test_exact_ties_go_to_the_smallest_value(which):
    y = labelvote_ref.label_volume(SRC, 21)
    m = labelvote_ref.shift_matrix(labelvote_ref.TIE_SHIFTS[which])
    val, wt = labelvote_ref.taps(y, m, SRC)
    assert set(np.unique(wt).tolist()) == ({0.0, 0.5} if which == 'w' else {0.125})      # exact weights, so exact ties
    lab, margin = labelvote_ref.label_vote(y, m, SRC)
    fov = conform_ref.inside(m, SRC, SRC)
    tie = labelvote_ref.tied(y, m, SRC)
    print('%s: %d exactly tied voxels of %d' % (which, int(tie.sum()), tie.size))
    assert tie.sum() >= 100 and not (tie & ~fov).any()
    assert not ((margin > 0) & (margin < 1e-9)).any()                  # tied exactly or clearly decided
    # the weight of every value by itself, and the smallest of those that reach the maximum
    totals = np.stack([np.where(val == v, wt, 0.0).sum(axis=0) for v in labelvote_ref.VALUES])
    smallest = np.array(labelvote_ref.VALUES)[np.argmax(totals == totals.max(axis=0), axis=0)]
    assert (totals == totals.max(axis=0)).sum(axis=0)[tie].min() >= 2
    assert np.array_equal(lab[fov], smallest.astype(np.float32)[fov])


# ---- host logic of preprocess --conform ----
def P():
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    return preprocess


def test_canvas_layout():
    size, offsets = P().canvas_layout([(10, 7, 5), (7, 7, 8), (9, 3, 8)])
    assert size == (10, 7, 8)
    assert offsets == [(0, 0, 1), (1, 0, 0), (0, 2, 0)]                  # 8 - 5 = 3: one plane below, two above
    assert P().canvas_layout([(4, 5, 6)]) == ((4, 5, 6), [(0, 0, 0)])
    for bad in ([], [(1, 2)], [(0, 1, 1)]):
        with pytest.raises(ValueError):
            P().canvas_layout(bad)


def test_truth_follows():
    lps = np.array([[-1.0, 0, 0, 90], [0, -1, 0, 126], [0, 0, 1, -72], [0, 0, 0, 1]])
    moved = lps.copy()
    moved[0, 3] += 3.0
    nearly = moved.copy()
    nearly[1, 3] += 5e-4
    off = lps.copy()
    off[2, 3] += 0.4
    shapes, affines = [(9, 8, 7), (9, 8, 7)], [lps, moved]
    f = P().truth_follows
    assert f(shapes, affines, (9, 8, 7), lps) == 0
    assert f(shapes, affines, (9, 8, 7), moved) == 1 and f(shapes, affines, (9, 8, 7), nearly) == 1
    assert f(shapes, affines, (9, 8, 7), off) is None
    assert f(shapes, affines, (9, 8, 6), lps) is None                   # the affine of the first, another shape
    assert f([(9, 8, 6), (9, 8, 7)], [lps, lps], (9, 8, 7), lps) == 1   # the shape decides among equal affines
    assert f(shapes, [lps, lps], (9, 8, 7), lps) == 0                   # on several: the first one


def saved(obj):
    buf = io.BytesIO()
    np.save(buf, obj)
    return buf.getvalue()


def test_record_without_geometry_is_unchanged_and_with_it_round_trips(tmp_path):
    p = P()
    size = {'h': 5, 'w': 6, 'd': 7, 'c': 2}
    mean, std = np.arange(2.0).reshape(1, 1, 1, 2), np.ones((1, 1, 1, 2))
    old = {'size': size, 'norm': {'mean': mean, 'std': std}}
    assert saved(p.prepro_record(size, mean, std)) == saved(old) == saved(p.prepro_record(size, mean, std, geometry=None))
    np.save(str(tmp_path / 'old.npy'), old)
    assert p.load_geometry(str(tmp_path / 'old.npy')) is None
    spec = p.GeometrySpec('RAS', 'nearest', {'bounds': (12.5, 7.0), 'bins': 16})
    rec = p.prepro_record(size, mean, std, geometry=spec)
    assert rec['geometry'] == {'orientation': 'RAS', 'spacing': (1.0, 1.0, 1.0), 'label_interp': 'nearest',
                               'coregister': {'bounds': (12.5, 7.0), 'bins': 16}}
    assert {k: v for k, v in rec.items() if k != 'geometry'} == old
    np.save(str(tmp_path / 'new.npy'), rec)
    assert p.load_geometry(str(tmp_path / 'new.npy')) == spec
    np.save(str(tmp_path / 'plain.npy'), p.prepro_record(size, mean, std, geometry=p.GeometrySpec()))
    assert p.load_geometry(str(tmp_path / 'plain.npy')) == p.GeometrySpec('LPS', 'vote', None)
    for bad in (p.GeometrySpec('LPX'), p.GeometrySpec(label_interp='cubic'), p.GeometrySpec(coregister={'bounds': (0.0, 5.0), 'bins': 8}),
                p.GeometrySpec(coregister={'bounds': (3.0, 5.0), 'bins': 1}), 'LPS'):
        with pytest.raises(ValueError):
            p.check_geometry(bad)
    rec['geometry']['spacing'] = (1.0, 1.0, 2.0)
    np.save(str(tmp_path / 'two.npy'), rec)
    with pytest.raises(ValueError, match='two.npy'):
        p.load_geometry(str(tmp_path / 'two.npy'))


PRE = ['--in_locs', 'a', '--modalities', 't1ce,flair', '--truth', 'seg']
TST = ['--in_locs', 'a', '--modalities', 't1ce,flair', '--tumor_prepro', 'p', '--tumor_model', 'm']


def refusal(parse, argv, capsys):
    with pytest.raises(SystemExit):
        parse(argv)
    return capsys.readouterr().err.split('error: ', 1)[1]


def test_both_parsers_share_the_geometry_flags(capsys):
    from bts_amd import test as T
    p = P()
    plain = p.parse_args(PRE)
    assert not any(hasattr(plain, k) for k in ('conform', 'coregister', 'coregister_max_mm', 'coregister_max_deg', 'coregister_bins',
                                               'label_interp'))
    assert p.geometry_spec(plain) is None
    assert p.geometry_spec(p.parse_args(PRE + ['--conform'])) == p.GeometrySpec('LPS', 'vote', None)
    assert p.geometry_spec(p.parse_args(PRE + ['--conform', 'ras', '--label_interp', 'nearest'])) == p.GeometrySpec('RAS', 'nearest', None)
    full = ['--conform', 'RAS', '--coregister', '--coregister_max_mm', '12.5', '--coregister_max_deg', '7', '--coregister_bins', '16']
    assert p.geometry_spec(p.parse_args(PRE + full)) == p.GeometrySpec('RAS', 'vote', {'bounds': (12.5, 7.0), 'bins': 16})
    assert T.coregister_kwargs(T.parse_args(TST + full)) == {'bounds': (12.5, 7.0), 'bins': 16}
    assert p.geometry_spec(p.parse_args(PRE + ['--conform', '--coregister'])).coregister == {'bounds': (30.0, 20.0), 'bins': 32}
    assert T.coregister_kwargs is p.coregister_kwargs and T.COREGISTER_DEFAULTS is p.COREGISTER_DEFAULTS
    for extra in (['--coregister'], ['--conform', '--coregister_bins', '16'], ['--conform', '--coregister', '--coregister_max_mm', '0'],
                  ['--conform', '--coregister', '--coregister_max_mm', 'nan'], ['--conform', '--coregister', '--coregister_max_deg', '181'],
                  ['--conform', '--coregister', '--coregister_bins', '65'], ['--conform', 'LPX']):
        a, b = refusal(p.parse_args, PRE + extra, capsys), refusal(T.parse_args, TST + extra, capsys)
        assert a == b and a.strip(), extra
    assert '--label_interp needs --conform' in refusal(p.parse_args, PRE + ['--label_interp', 'vote'], capsys)
    refusal(p.parse_args, PRE + ['--conform', '--label_interp', 'cubic'], capsys)
    refusal(T.parse_args, TST + ['--conform', '--label_interp', 'vote'], capsys)      # a flag of the training side alone
