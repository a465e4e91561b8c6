"""CPU: the host side of conforming a scan to an oriented grid by its affine -- the float64 restatements of tests/conform_ref.py pinned to
SciPy and numpy, the NIfTI geometry of bts_amd.nifti (qform, affine selection, orientation codes), infer.Conformer.plan, the argument
checks of the two entry points and the --conform flag.

The resampling restatement is compared with scipy.ndimage.affine_transform(mode='reflect') per channel INSIDE the source's field of view
(outside it SciPy reflects on, the restatement and the kernel give 0): to 1e-12 * max|ref| at order 3, exactly at orders 0 and 1 away
from coordinates within 1e-9 of a rounding tie or a face.  Every matrix keeps at least 30 % of the output inside the field of view.
SciPy reflects a negative coordinate before it forms the taps, the kernel reflects the tap indices (conform_ref: scipy_mirror): the exact
comparison runs with the flag set, and the plain restatement must then equal the flagged one bit for bit wherever no coordinate is negative.
"""
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import conform_ref  # noqa: E402

import bts_amd  # noqa: E402,F401
from bts_amd import infer, nifti  # noqa: E402

from conform_ref import OUT, SRC, matrices, rotation, volume  # noqa: E402


@pytest.mark.parametrize('name', ['oblique', 'anisotropic', 'permuting', 'integer'])
@pytest.mark.parametrize('order', [0, 1, 3])
def test_resampling_restatement_equals_scipy_inside_the_field_of_view(name, order):
    ndi = pytest.importorskip('scipy.ndimage')
    m = matrices()[name]
    out = (37, 19, 23) if name == 'integer' else OUT
    x = volume(SRC, 2, 5)
    fov = conform_ref.inside(m, out, SRC)
    print('%s: %.1f %% of the output inside the field of view' % (name, 100.0 * fov.mean()))
    assert fov.mean() >= 0.30
    ref = np.stack([ndi.affine_transform(x[..., c].astype(np.float64), m[:, :3], offset=m[:, 3], output_shape=out, order=order,
                                         mode='reflect') for c in range(x.shape[-1])], -1)
    got = conform_ref.affine_resample(x, m, out, order, np.float64, scipy_mirror=True)
    assert got.shape == ref.shape
    assert float(np.abs(got[~fov]).max(initial=0.0)) == 0.0
    sel = fov & ~conform_ref.near_a_decision(m, out, SRC, order, eps=1e-9)
    assert sel.sum() >= 0.999 * fov.sum()
    err = float(np.abs(got[sel] - ref[sel]).max())
    print('%s order %d: max deviation %.3g of max|ref| %.3g' % (name, order, err, np.abs(ref).max()))
    if order == 3:
        assert err <= 1e-12 * np.abs(ref).max()
    else:
        assert err == 0.0
    # the restatement the GPU tests use reflects tap indices only, as the kernel does: the same bits wherever no coordinate is negative,
    # and the last bit of the weights elsewhere
    plain = conform_ref.affine_resample(x, m, out, order, np.float64)
    s = conform_ref.coordinates(m, out)
    mirrored = (s < 0).any(axis=0)
    assert np.array_equal(plain[~mirrored], got[~mirrored])
    assert float(np.abs(plain - got).max()) <= 1e-12 * np.abs(ref).max()
    if name != 'integer':
        assert (mirrored & fov).sum() > 0


def test_integer_map_is_the_reorientation():
    """an integer signed permutation resamples, at orders 0 and 1, to exactly the reoriented array on every voxel"""
    m = matrices()['integer']
    x = volume(SRC, 2, 6)
    want = conform_ref.reorient(x, (2, 0, 1), (False, True, False))
    assert conform_ref.inside(m, (37, 19, 23), SRC).all()
    for order in (0, 1):
        assert np.array_equal(conform_ref.affine_resample(x, m, (37, 19, 23), order, np.float32), want)


def test_reorientation_restatement_is_transpose_and_flip():
    x = volume((5, 6, 7), 2, 1)
    seen = set()
    for src in conform_ref.all_codes():
        perm, flip = conform_ref.reorientation(src, 'LPS')
        seen.add((perm, flip))
        want = np.flip(np.transpose(x, perm + (3,)), [a for a in range(3) if flip[a]])
        assert np.array_equal(conform_ref.reorient(x, perm, flip), want), src
    assert len(seen) == 48


def test_orientation_codes_of_all_signed_permutations():
    codes = conform_ref.all_codes()
    assert len(set(codes)) == 48
    rng = np.random.default_rng(2)
    for code in codes:
        a = np.eye(4)
        a[:3, :3] = conform_ref.signed_permutation_affine(code, (0.7, 1.0, 2.5))
        a[:3, 3] = rng.uniform(-90, 90, 3)
        assert nifti.orientation(a) == code == conform_ref.orientation(a)
        for _ in range(4):
            b = a.copy()
            b[:3, :3] = rotation(rng.standard_normal(3), rng.uniform(-30.0, 30.0)) @ a[:3, :3]
            assert nifti.orientation(b) == code, (code, b)
    assert nifti.orientation(np.diag([-1.0, -1.0, 1.0, 1.0])) == 'LPS' and nifti.orientation(np.eye(4)) == 'RAS'
    tie = np.eye(4)
    tie[:3, :3] = rotation((0, 0, 1), 45.0)                    # |cos| == |sin|: lowest column, then lowest row
    assert nifti.orientation(tie) == conform_ref.orientation(tie)


def test_orientation_refuses_a_singular_affine():
    for bad in (np.zeros((4, 4)), np.diag([1.0, 0.0, 1.0, 1.0]), np.array([[1.0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]),
                np.diag([1.0, np.nan, 1.0, 1.0]), np.diag([1.0, np.inf, 1.0, 1.0])):
        with pytest.raises(ValueError):
            nifti.orientation(bad)


def test_reorientation_between_codes():
    for src in conform_ref.all_codes():
        for dst in ('LPS', 'RAS', 'ASL', 'IPR'):
            assert nifti.reorientation(src, dst) == conform_ref.reorientation(src, dst)
    assert nifti.reorientation('RAS', 'LPS') == ((0, 1, 2), (True, True, False))
    assert nifti.reorientation('LPS', 'LPS') == ((0, 1, 2), (False, False, False))
    assert nifti.reorientation('ASL', 'LPS') == ((2, 0, 1), (False, True, False))
    for bad in ('LPSS', 'LP', 'LRS', 'XYZ', 'lps', ''):
        with pytest.raises(ValueError):
            nifti.reorientation(bad, 'LPS')
        with pytest.raises(ValueError):
            nifti.reorientation('LPS', bad)


R2 = np.sqrt(0.5)
QFORM_CASES = [  # quatern (b, c, d), qfac, the rotation it stands for
    ((0.0, 0.0, 0.0), 1.0, np.eye(3)),
    ((R2, 0.0, 0.0), 1.0, np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])),          # a quarter turn about x
    ((0.0, R2, 0.0), 1.0, np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])),          # about y
    ((0.0, 0.0, R2), 1.0, np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])),          # about z
    ((0.0, 0.0, R2), -1.0, np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, -1]])),        # the same with qfac = -1: the third column reversed
]


def write_with_qform(path, array, srow_affine, quatern, qoffset, pixdim123, qfac, qform_code, sform_code):
    """nifti.save, then the qform fields patched into the header"""
    nifti.save(path, array, srow_affine)
    raw = bytearray(open(path, 'rb').read())
    struct.pack_into('<4f', raw, 76, qfac, *pixdim123)
    struct.pack_into('<2h', raw, 252, qform_code, sform_code)
    struct.pack_into('<3f', raw, 256, *quatern)
    struct.pack_into('<3f', raw, 268, *qoffset)
    open(path, 'wb').write(bytes(raw))


@pytest.mark.parametrize('case', range(len(QFORM_CASES)))
def test_qform_affine_by_hand(tmp_path, case):
    quatern, qfac, rot = QFORM_CASES[case]
    pix, off = (2.0, 3.0, 4.0), (-10.0, 20.5, 30.0)
    want = np.eye(4)
    want[:3, :3] = rot * np.array(pix)
    want[:3, 3] = off
    path = str(tmp_path / 'q.nii')
    srows = np.diag([5.0, 6.0, 7.0, 1.0])
    write_with_qform(path, np.zeros((3, 4, 5), np.float32), srows, quatern, off, pix, qfac, 1, 0)
    data, header = nifti.load(path)
    assert data.shape == (3, 4, 5)
    assert np.allclose(header['quatern'], quatern, atol=1e-7) and np.allclose(header['qoffset'], off) and header['qfac'] == qfac
    assert np.array_equal(header['affine'], srows.astype(np.float32))                    # `affine` stays the srow matrix
    got = nifti.qform_affine(header)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-6
    assert np.abs(conform_ref.qform_affine(header['quatern'], header['qoffset'], header['pixdim'], header['qfac']) - got).max() <= 1e-12
    assert np.array_equal(nifti.best_affine(header), got)                                # sform_code 0, qform_code 1


def test_best_affine_precedence_and_refusal(tmp_path):
    path = str(tmp_path / 'b.nii')
    srows = np.array([[0.0, 0, 2, 1], [-1, 0, 0, 2], [0, 3, 0, 3], [0, 0, 0, 1]])
    args = (np.zeros((3, 4, 5), np.int16), srows, (0.0, 0.0, R2), (1.0, 2.0, 3.0), (1.0, 1.0, 1.0), 1.0)
    write_with_qform(path, *args, 1, 2)
    _, h = nifti.load(path)
    assert np.array_equal(nifti.best_affine(h), srows)                                  # a sform wins over a qform
    write_with_qform(path, *args, 0, 1)
    assert np.array_equal(nifti.best_affine(nifti.load(path)[1]), srows)
    write_with_qform(path, *args, 2, 0)
    _, h = nifti.load(path)
    assert np.array_equal(nifti.best_affine(h), nifti.qform_affine(h)) and nifti.orientation(nifti.best_affine(h)) == 'ALS'
    write_with_qform(path, *args, 0, 0)
    _, h = nifti.load(path)
    with pytest.raises(ValueError, match='sform_code = 0 and qform_code = 0'):
        nifti.best_affine(h)
    _, plain = nifti.load(path)
    assert {'quatern', 'qoffset', 'qfac'} <= set(plain) and plain['qfac'] == 1.0


LPS = np.array([[-1.0, 0, 0, 90], [0, -1, 0, 126], [0, 0, 1, -72], [0, 0, 0, 1]])


def ras_copy_affine(shape):
    """the affine of the same scan stored with the first two array axes reversed"""
    v = np.eye(4)
    v[0, 0], v[0, 3], v[1, 1], v[1, 3] = -1.0, shape[0] - 1, -1.0, shape[1] - 1
    return LPS @ v


def test_plan_of_an_lps_scan_is_the_scan_itself():
    p = infer.Conformer().plan([SRC], [LPS])
    assert p['shape'] == SRC and p['code'] == 'LPS' and p['groups'] == [[0]]
    assert np.array_equal(p['matrices'][0], np.eye(4)[:3]) and np.array_equal(p['target_affine'], LPS)
    assert p['reorient'] == [((0, 1, 2), (False, False, False))]
    f32 = LPS.astype(np.float32) * np.float32(1.0000001)                                 # srows as a float32 header holds them
    p = infer.Conformer().plan([SRC], [f32])
    assert p['reorient'] == [((0, 1, 2), (False, False, False))] and np.array_equal(p['matrices'][0], np.eye(4)[:3])


def test_plan_of_a_ras_copy_is_a_two_flip_reorientation():
    ras = ras_copy_affine(SRC)
    assert nifti.orientation(ras) == 'RAS'
    p = infer.Conformer().plan([SRC], [ras])
    assert p['shape'] == SRC and p['code'] == 'RAS'
    assert p['reorient'] == [((0, 1, 2), (True, True, False))]
    assert np.abs(p['target_affine'] - LPS).max() <= 1e-12                               # the target grid IS the LPS scan's
    want = np.array([[-1.0, 0, 0, SRC[0] - 1], [0, -1, 0, SRC[1] - 1], [0, 0, 1, 0]])
    assert np.array_equal(p['matrices'][0], want)


def test_plan_groups_modalities_by_grid():
    c = infer.Conformer()
    p = c.plan([SRC, SRC], [LPS, LPS.copy()])
    assert p['groups'] == [[0, 1]] and len(p['reorient']) == 1
    shifted = LPS.copy()
    shifted[0, 3] += 2.5                                                                 # the same axes, 2.5 mm along x
    p = c.plan([SRC, SRC, SRC], [LPS, shifted, LPS])
    assert p['groups'] == [[0, 2], [1]]
    assert p['reorient'][0] == ((0, 1, 2), (False, False, False)) and p['reorient'][1] is None
    assert np.allclose(p['matrices'][1], np.array([[1.0, 0, 0, 2.5], [0, 1, 0, 0], [0, 0, 1, 0]]), atol=1e-12)
    p = c.plan([SRC, (19, 23, 36)], [LPS, LPS])                                          # another extent: a launch of its own
    assert p['groups'] == [[0], [1]] and p['reorient'][1] is None
    whole = LPS.copy()
    whole[2, 3] += 3.0                                                                   # whole voxels off: no copy of the whole array
    assert c.plan([SRC, SRC], [LPS, whole])['reorient'][1] is None


def test_plan_matches_the_restatement_on_general_scans():
    rng = np.random.default_rng(7)
    for code, scale, spacing in (('ASL', (1.0, 1.0, 2.0), (1.0, 1.0, 1.0)), ('RIP', (0.8, 1.3, 2.2), (1.0, 1.0, 1.0)),
                                 ('PSR', (0.5, 0.5, 3.0), (1.5, 1.0, 0.75))):
        a = np.eye(4)
        a[:3, :3] = rotation(rng.standard_normal(3), 12.0) @ conform_ref.signed_permutation_affine(code, scale)
        a[:3, 3] = rng.uniform(-50, 50, 3)
        other = a.copy()
        other[:3, :3] = rotation((0, 0, 1), 3.0) @ a[:3, :3] * 1.1
        shapes = [(19, 23, 37), (20, 21, 30)]
        p = infer.Conformer('LPS', spacing).plan(shapes, [a, other])
        shape, target, mats = conform_ref.plan(shapes, [a, other], 'LPS', spacing)
        assert p['shape'] == shape and p['code'] == code and p['groups'] == [[0], [1]]
        assert np.abs(p['target_affine'] - target).max() <= 1e-9
        for got, want in zip(p['matrices'], mats):
            assert np.abs(got - want).max() <= 1e-9
        assert nifti.orientation(p['target_affine']) == 'LPS'
        assert np.allclose(np.linalg.norm(p['target_affine'][:3, :3], axis=0), spacing)
        # the outer faces coincide: the target's first face is the reference's first or last face along that axis
        for a_out in range(3):
            lo = np.array([-0.5 if k == a_out else 0.0 for k in range(3)] + [1.0])
            src_axis = int(np.argmax(np.abs(p['voxel_map'][:3, a_out])))
            s = (p['voxel_map'] @ lo)[src_axis]
            assert min(abs(s + 0.5), abs(s - (shapes[0][src_axis] - 0.5))) <= 1e-9
    assert infer.Conformer('LPS').plan([(19, 23, 37)], [np.diag([-1.0, -1.0, 2.0, 1.0])])['shape'] == (19, 23, 74)


def test_signed_permutation_tolerances():
    m = np.array([[0.0, -1.0, 0.0, 22.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    assert infer.signed_permutation(m, (23, 19, 37), (19, 23, 37)) == ((1, 0, 2), (False, True, False))
    assert infer.signed_permutation(m, (23, 19, 37), (19, 23, 36)) is None              # extents
    near = m.copy()
    near[0, 3] += 5e-4
    assert infer.signed_permutation(near, (23, 19, 37), (19, 23, 37)) is not None
    near[0, 3] += 1e-3
    assert infer.signed_permutation(near, (23, 19, 37), (19, 23, 37)) is None            # a corner more than 1e-3 voxel off
    bent = m.copy()
    bent[1, 1] = 1e-5
    assert infer.signed_permutation(bent, (23, 19, 37), (19, 23, 37)) is None            # an entry more than 1e-6 off


def test_conformer_refuses_bad_arguments():
    with pytest.raises(ValueError):
        infer.Conformer('LLS')
    with pytest.raises(ValueError):
        infer.Conformer(order=2)
    with pytest.raises(ValueError):
        infer.Conformer(spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        infer.Conformer().plan([SRC], [LPS, LPS])
    with pytest.raises(ValueError):
        infer.Conformer().plan([SRC], [np.zeros((4, 4))])
    with pytest.raises(RuntimeError):
        infer.Conformer().reverse(None)
    with pytest.raises(ValueError, match='geometry'):
        infer.segment_scan(None, None, None, None, None, 8, geometry=(None, [], []))


def test_entry_points_check_their_arguments_without_a_gpu():
    from bts_amd._lib import lib
    L = lib()
    one = 1                                                                              # any non-null address: nothing is launched
    assert L._bts_reorient3d(one, 2, 0, 4, 4, 2, 0, 1, 2, 0, None) == -1                 # extent < 1
    assert L._bts_reorient3d(one, 2, 4, 4, 4, 9, 0, 1, 2, 0, None) == -1                 # C > 8
    assert L._bts_reorient3d(one, 2, 4, 4, 4, 2, 0, 1, 1, 0, None) == -1                 # no permutation
    assert L._bts_reorient3d(one, 2, 4, 4, 4, 2, 0, 1, 3, 0, None) == -1
    assert L._bts_reorient3d(one, 2, 4, 4, 4, 2, 0, 1, 2, 8, None) == -1                 # flip bits
    assert L._bts_reorient3d(None, 2, 4, 4, 4, 2, 0, 1, 2, 0, None) == -1                # null
    assert L._bts_reorient3d(one, one, 4, 4, 4, 2, 0, 1, 2, 0, None) == -1               # in place
    import ctypes
    m = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    good = dict(coef=16, Ds=4, Hs=4, Ws=4, C=2, dst=32, ld=2, c0=0, bmask=None, Do=4, Ho=4, Wo=4, Dp=4, Hp=4, Wp=4, m=m, order=1)

    def call(**kw):
        a = dict(good, **kw)
        return L._bts_affine_resample3d(a['coef'], a['Ds'], a['Hs'], a['Ws'], a['C'], a['dst'], a['ld'], a['c0'], a['bmask'], a['Do'],
                                        a['Ho'], a['Wo'], a['Dp'], a['Hp'], a['Wp'], a['m'], a['order'], None)
    assert call(Ds=0) == -1 and call(Wo=0) == -1 and call(C=0) == -1 and call(C=9) == -1
    assert call(Hp=3) == -1                                                              # pad < out
    assert call(ld=1) == -1 and call(c0=1) == -1 and call(c0=-1) == -1                   # ld < C, channels past ld
    assert call(coef=None) == -1 and call(dst=None) == -1 and call(m=None) == -1
    assert call(bmask=64, ld=4) == -1                                                    # a mask of some of the channels
    assert call(order=2) == -3
    assert call(coef=4) == -2                                                            # C == 2 is read as float2


def test_command_line_accepts_conform():
    from bts_amd import test as cli
    base = ['--in_locs', 'a', '--modalities', 't1ce,flair', '--tumor_prepro', 'p.npy', '--tumor_model', 'm']
    assert not hasattr(cli.parse_args(base), 'conform')                                  # absent: off
    assert cli.parse_args(base + ['--conform']).conform == 'LPS'
    assert cli.parse_args(base + ['--conform', 'RAS']).conform == 'RAS'
    assert cli.parse_args(base + ['--conform', '--order', '1']).conform == 'LPS'
    with pytest.raises(SystemExit):
        cli.parse_args(base + ['--conform', 'RRS'])


def test_decode_case_in_conform_mode(tmp_path):
    from bts_amd import test as cli
    case = tmp_path / 'case'
    case.mkdir()
    rng = np.random.default_rng(3)
    t1 = rng.uniform(0, 100, (5, 6, 7)).astype(np.float32)
    fl = rng.uniform(0, 100, (6, 6, 8)).astype(np.float32)                               # another grid
    other = LPS.copy()
    other[:3, :3] *= 0.9
    nifti.save(str(case / 'x_t1.nii'), t1, LPS)
    nifti.save(str(case / 'x_flair.nii.gz'), fl, other)
    nifti.save(str(case / 'x_seg.nii'), np.ones((5, 6, 7), np.uint8), LPS)
    out = cli.decode_case(str(case), ['t1', 'flair'], 'seg', True)
    assert [v.shape for v in out['vols']] == [(7, 6, 5), (8, 6, 6)]
    assert np.array_equal(out['affines'][0], LPS) and np.allclose(out['affines'][1], other) and out['truth'].shape == (7, 6, 5)
    assert 'affines' not in cli.decode_case(str(case), ['t1'], 'seg')                    # without the flag: as before
    moved = LPS.copy()
    moved[1, 3] += 0.5
    nifti.save(str(case / 'x_seg.nii'), np.ones((5, 6, 7), np.uint8), moved)
    assert 'refused' in cli.decode_case(str(case), ['t1', 'flair'], 'seg', True)
    nifti.save(str(case / 'x_seg.nii'), np.ones((5, 6, 8), np.uint8), LPS)
    assert 'another shape' in cli.decode_case(str(case), ['t1', 'flair'], 'seg', True)['refused']
    write_with_qform(str(case / 'x_t1.nii'), t1, LPS, (0, 0, 0), (0, 0, 0), (1, 1, 1), 1.0, 0, 0)
    assert 'no orientation' in cli.decode_case(str(case), ['t1', 'flair'], '', True)['refused']
