"""-m gpu: `python -m bts_amd.preprocess --conform` on three small synthetic cases written as NIfTI files -- A: LPS at 1 mm; B: the same
anatomy stored RAS; C: another extent at 1 x 1 x 2 mm whose second modality, and the truth drawn on it, lie on a shifted grid of their own
-- and `python -m bts_amd.test` following the geometry that prepro.npy records.

Images are compared bit for bit with what infer.Conformer and the normalisation give when called directly; labels with the float64
restatement tests/labelvote_ref.py (vote) and tests/conform_ref.py (order 0) through the plan's matrix, on every voxel: the test shows
first that the restatement holds no voxel of C whose decision hangs on a last bit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import conform_ref  # noqa: E402
import coreg_ref  # noqa: E402
import labelvote_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LPS = np.array([[-1.0, 0, 0, 90], [0, -1, 0, 126], [0, 0, 1, -72], [0, 0, 0, 1]])
SHAPE_A = (24, 28, 20)
GRID_C0, GRID_C1 = (20, 24, 9), (22, 21, 10)
MODS = ('t1ce', 'flair')


def dev():
    return torch.device('cuda', 0)


def grids_of_c():
    g0 = np.eye(4)
    g0[:3, :3] = np.diag([-1.0, -1.0, 2.0])
    g0[:3, 3] = (10.0, 12.0, -9.0)
    g1 = g0.copy()
    g1[:3, 3] += (2.3, -2.7, -1.2)                                      # 2.3 and 2.7 voxels in the plane, 0.6 of a slice
    return g0, g1


def anatomy(shape, seed, channel):
    """a textured head, strictly positive inside an ellipsoid and exactly zero around it"""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    rng = np.random.default_rng(seed)
    tex = 0.65 + 0.3 * np.sin(5.0 * g[0] + 1.0 + channel) * np.cos(4.0 * g[1] + 2.0) * np.sin(6.0 * g[2] + 0.5) + 0.02 * rng.random(shape)
    r2 = (g[0] / 0.8) ** 2 + (g[1] / 0.7) ** 2 + (g[2] / 0.75) ** 2
    return np.where(r2 < 1.0, tex * (160.0 + 30.0 * channel), 0.0).astype(np.float32)


def ras_copy(array, affine):
    """the same scan stored with the first two array axes reversed"""
    v = np.eye(4)
    v[0, 0], v[0, 3], v[1, 1], v[1, 3] = -1.0, array.shape[0] - 1, -1.0, array.shape[1] - 1
    return np.ascontiguousarray(array[::-1, ::-1]), affine @ v


def box_of(x):
    """the full occupancy box of a (D,H,W,C) array: [first occupied plane, last occupied plane + 1) per axis"""
    lo, hi = [], []
    for a in range(3):
        idx = np.nonzero((x != 0).any(axis=tuple(b for b in range(4) if b != a)))[0]
        lo.append(int(idx[0]))
        hi.append(int(idx[-1]) + 1)
    return lo, hi


def on_canvas(v, box, size, offset):
    lo, hi = box
    out = np.zeros(tuple(size) + v.shape[3:], dtype=v.dtype)
    out[offset[0]:offset[0] + hi[0] - lo[0], offset[1]:offset[1] + hi[1] - lo[1], offset[2]:offset[2] + hi[2] - lo[2]] = \
        v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    return out


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    """the three cases on disk, and what was written: {name: ([modality arrays], [affines], truth array, truth affine)}"""
    import bts_amd  # noqa: F401
    from bts_amd import nifti
    root = tmp_path_factory.mktemp('conform')
    a = [anatomy(SHAPE_A, 1, c) for c in range(2)]
    ya = labelvote_ref.label_volume(SHAPE_A, 31)
    g0, g1 = grids_of_c()
    written = {'a': (a, [LPS, LPS], ya, LPS),
               'b': ([ras_copy(v, LPS)[0] for v in a], [ras_copy(a[0], LPS)[1]] * 2, ras_copy(ya, LPS)[0], ras_copy(ya, LPS)[1]),
               'c': ([anatomy(GRID_C0, 2, 0), anatomy(GRID_C1, 3, 1)], [g0, g1], labelvote_ref.label_volume(GRID_C1, 33), g1)}
    for where, names in (('data', 'abc'), ('only_c', 'c')):
        for name in names:
            vols, affs, y, ya_aff = written[name]
            os.makedirs(str(root / where / name))
            for mod, v, aff in zip(MODS, vols, affs):
                nifti.save(str(root / where / name / ('s_%s.nii.gz' % mod)), v, aff)
            if where == 'data':
                nifti.save(str(root / where / name / 's_seg.nii.gz'), y, ya_aff)
    return root, written


def read_case(root, name):
    """as the files give them back: ([arrays], [best affines], truth, truth affine)"""
    from bts_amd import nifti
    vols, affs = [], []
    for mod in MODS + ('seg',):
        data, header = nifti.load(str(root / 'data' / name / ('s_%s.nii.gz' % mod)))
        vols.append(np.asarray(data).astype(np.float32))
        affs.append(nifti.best_affine(header))
    return vols[:2], affs[:2], vols[2], affs[2]


@pytest.fixture(scope='module')
def conformed(cases):
    """one run of the command with --conform, and the direct restatement of every case: computed once, shared"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    from bts_amd import preprocess as P
    root, _ = cases
    out = str(root / 'out')
    base = ['--in_locs', str(root / 'data'), '--modalities', ','.join(MODS), '--truth', 'seg']
    assert P.main(base + ['--out_loc', out, '--conform']) == 0
    direct = {}
    for name in 'abc':
        vols, affs, y, y_aff = read_case(root, name)
        conf = infer.Conformer('LPS')
        x, _, shape = conf.forward(vols, affs)
        direct[name] = {'x': x.cpu().numpy(), 'plan': conf.last, 'shape': tuple(shape), 'truth': y, 'truth_affine': y_aff, 'affines': affs,
                        'shapes': [v.shape for v in vols]}
        direct[name]['box'] = box_of(direct[name]['x'])
    extents = [[h - l for l, h in zip(*direct[n]['box'])] for n in 'abc']
    size, offsets = P.canvas_layout(extents)
    return root, base, out, direct, size, dict(zip('abc', offsets))


def example(out, k):
    with np.load(os.path.join(out, 'train', '%d.npz' % k)) as f:
        return f['x'], f['y']


def test_without_conform_the_differing_shapes_are_refused(cases):
    import bts_amd  # noqa: F401
    from bts_amd import preprocess as P
    root, _ = cases
    with pytest.raises(ValueError, match='differ'):
        P.preprocess([str(root / 'data')], list(MODS), 'seg', str(root / 'plain_out'))


def test_lps_and_ras_storage_give_the_same_examples(conformed):
    root, base, out, direct, size, offsets = conformed
    (xa, ya), (xb, yb) = example(out, 1), example(out, 2)
    assert xa.shape == tuple(size) + (2,) and ya.shape == tuple(size) + (1,) and xa.dtype == ya.dtype == np.float32
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
    assert direct['b']['plan']['code'] == 'RAS' and np.array_equal(direct['a']['x'], direct['b']['x'])
    # and they are A's own arrays: the labels as stored (4 -> 3), on the canvas
    _, _, y, _ = read_case(root, 'a')
    want = on_canvas(np.where(y >= 4, 3.0, y).astype(np.float32)[..., None], direct['a']['box'], size, offsets['a'])
    assert np.array_equal(ya, want) and set(np.unique(ya).tolist()) == {0.0, 1.0, 2.0, 3.0}


def test_record_holds_the_geometry_and_the_largest_box(conformed):
    from bts_amd import preprocess as P
    root, base, out, direct, size, offsets = conformed
    rec = np.load(os.path.join(out, 'prepro.npy'), allow_pickle=True).item()
    assert rec['geometry'] == {'orientation': 'LPS', 'spacing': (1.0, 1.0, 1.0), 'label_interp': 'vote', 'coregister': None}
    assert P.load_geometry(os.path.join(out, 'prepro.npy')) == P.GeometrySpec('LPS', 'vote', None)
    boxes = [direct[n]['box'] for n in 'abc']
    assert rec['size'] == {'h': size[0], 'w': size[1], 'd': size[2], 'c': 2}
    assert tuple(size) == tuple(max(h[a] - l[a] for l, h in boxes) for a in range(3))
    assert direct['c']['shape'] == (20, 24, 18)
    print('boxes %s, size %s, offsets %s' % (boxes, size, offsets))
    assert any(offsets[n] != (0, 0, 0) for n in 'abc')                  # some case is smaller than the canvas and sits inside it
    lo, hi = direct['a']['box']                                         # the full box: its last plane is occupied
    assert all(direct['a']['x'].take(hi[a] - 1, axis=a).any() for a in range(3))


def test_case_c_is_the_conformer_and_the_vote(conformed):
    from bts_amd import preprocess as P
    root, base, out, direct, size, offsets = conformed
    d = direct['c']
    assert d['plan']['reorient'] == [None, None] and d['plan']['code'] == 'LPS'
    _, mean, std = P.load_prepro(os.path.join(out, 'prepro.npy'))
    m_y = d['plan']['matrices'][1]                                      # the truth lies on the second modality's grid
    assert P.truth_follows(d['shapes'], d['affines'], d['truth'].shape, d['truth_affine']) == 1
    assert np.abs(m_y - (np.linalg.inv(d['truth_affine']) @ d['plan']['target_affine'])[:3]).max() <= 1e-12
    ref, margin = labelvote_ref.label_vote(d['truth'], m_y, d['shape'])
    fov = conform_ref.inside(m_y, d['shape'], d['truth'].shape)
    print('case C: smallest margin %.3g, %.0f %% inside the field of view' % (float(margin.min()), 100 * fov.mean()))
    assert float(margin.min()) >= 1e-9 and not conform_ref.near_a_decision(m_y, d['shape'], d['truth'].shape, 1, eps=1e-6).any()
    assert 0.5 < fov.mean() < 1.0
    y_want = on_canvas(np.where(ref >= 4, 3.0, ref).astype(np.float32)[..., None], d['box'], size, offsets['c'])
    x_canvas = torch.from_numpy(on_canvas(d['x'], d['box'], size, offsets['c'])).to(dev())
    x_want, y_norm = P.normalize_example(x_canvas, torch.from_numpy(y_want).to(dev()), mean, std)
    x, y = example(out, 3)
    assert np.array_equal(y, y_want) and np.array_equal(y_norm.cpu().numpy(), y_want)
    assert np.array_equal(x, x_want.cpu().numpy())
    assert set(np.unique(y).tolist()) == {0.0, 1.0, 2.0, 3.0}


def test_label_interp_nearest_gives_the_order_0_labels(conformed):
    import bts_amd  # noqa: F401
    from bts_amd import preprocess as P
    root, base, out, direct, size, offsets = conformed
    near_out = str(root / 'out_nearest')
    assert P.main(base + ['--out_loc', near_out, '--conform', 'LPS', '--label_interp', 'nearest']) == 0
    assert P.load_geometry(os.path.join(near_out, 'prepro.npy')) == P.GeometrySpec('LPS', 'nearest', None)
    d = direct['c']
    m_y = d['plan']['matrices'][1]
    assert not conform_ref.near_a_decision(m_y, d['shape'], d['truth'].shape, 0, eps=1e-6).any()
    ref = conform_ref.interpolate(d['truth'][..., None].astype(np.float64), m_y, d['shape'], 0)
    want = on_canvas(np.where(ref >= 4, 3.0, ref).astype(np.float32), d['box'], size, offsets['c'])
    x, y = example(near_out, 3)
    assert np.array_equal(y, want)
    xv, yv = example(out, 3)
    assert np.array_equal(x, xv)                                         # the images do not depend on the label rule
    differ = int((y != yv).sum())
    print('case C: nearest and vote differ on %d of %d voxels' % (differ, y.size))
    assert differ > 0
    for k in (1, 2):                                                     # exact reorientations: no rule is applied
        assert np.array_equal(example(near_out, k)[1], example(out, k)[1])


def test_the_test_command_follows_the_record(conformed, capsys):
    """python -m bts_amd.test on case C with the prepro.npy that preprocess wrote and NO --conform: one line says that the recorded
    geometry applies, and mask.nii is the one that --conform LPS gives"""
    import bts_amd  # noqa: F401
    from bts_amd import nifti
    from bts_amd import test as T
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    from oracle import torch_ref as O
    from segment_ref import randomised_params
    root, base, out, direct, size, offsets = conformed
    kw, res = dict(base_filters=8, groups=2, reduction=2, depth=3), 8
    padded = tuple(s + res - s % res for s in direct['c']['shape'])
    model = Model(**kw)
    model.build((1,) + padded + (2,))
    model.set_weights_from(randomised_params(O.default_config(**kw), padded, seed=5))
    save_checkpoint(str(root / 'tumor'), model)
    save_train_args(str(root / 'tumor'), {'model_args': dict(kw), 'crop_size': list(padded)})
    prepro = os.path.join(out, 'prepro.npy')
    argv = ['--in_locs', str(root / 'only_c'), '--modalities', ','.join(MODS), '--tumor_model', str(root / 'tumor'), '--tumor_prepro', prepro,
            '--workers', '0']
    capsys.readouterr()
    assert T.main(argv + ['--out_loc', str(root / 'followed')]) == 0
    text = capsys.readouterr().out
    line = 'Geometry (recorded by %s): conform to LPS at 1 mm' % prepro
    assert text.count(line) == 1 and 'c. Orientation LPS -> LPS, voxel size 1 x 1 x 2 mm, resampled at order 3' in text
    assert T.main(argv + ['--out_loc', str(root / 'given'), '--conform', 'LPS']) == 0
    text = capsys.readouterr().out
    assert 'Geometry (recorded' not in text and 'Warning' not in text
    assert T.main(argv + ['--out_loc', str(root / 'other'), '--conform', 'RAS']) == 0
    assert 'Warning: --conform RAS over the record of %s, whose examples were conformed to LPS' % prepro in capsys.readouterr().out
    a, ha = nifti.load(str(root / 'followed' / 'c' / 'mask.nii'))
    b, hb = nifti.load(str(root / 'given' / 'c' / 'mask.nii'))
    assert a.shape == GRID_C0 and np.array_equal(a, b) and np.array_equal(ha['affine'], hb['affine'])
    # an ensemble whose dumps disagree is refused, and the refusal names the member
    rec = np.load(prepro, allow_pickle=True).item()
    del rec['geometry']
    np.save(str(root / 'old.npy'), rec)
    two = [v for v in argv]
    two[two.index('--tumor_model') + 1] = '%s,%s' % (root / 'tumor', root / 'tumor')
    two[two.index('--tumor_prepro') + 1] = '%s,%s' % (prepro, root / 'old.npy')
    with pytest.raises(ValueError, match='old.npy'):
        T.main(two + ['--out_loc', str(root / 'two')])


def test_coregistration_moves_the_truth_with_its_modality():
    """the second modality lies on a grid of its own and shows the anatomy 3 mm from where its header says; the truth is drawn on that
    grid.  Whatever the registration finds, the truth's affine gets that modality's correction, and the labels are read through that
    modality's matrix of the plan"""
    import bts_amd  # noqa: F401
    from bts_amd import coreg
    from bts_amd import preprocess as P
    fs, ms = (28, 33, 25), (24, 37, 27)
    shrink = np.diag([1.0 / 6.0] * 3 + [1.0])                             # the phantom's 6 mm world stored as 1 mm headers
    a6 = coreg_ref.grid_affine(fs, (6.0,) * 3)
    moved = coreg.rigid_matrix((18.0, 0.0, 0.0, 0.0, 0.0, 0.0), (a6 @ np.array([13, 16, 12, 1.0]))[:3])      # 3 mm once shrunk
    f, a_f, m, a_m = coreg_ref.phantom_pair(fs, (6.0,) * 3, ms, (6.6, 5.4, 5.8), moved)
    affines = [shrink @ a_f, shrink @ a_m]
    truth = labelvote_ref.label_volume(ms, 41)
    vols = [torch.from_numpy(f).to(dev()), torch.from_numpy(m).to(dev())]
    reg = {'bounds': (6.0, 20.0), 'bins': 16}
    r = P.conform_case(vols, affines, torch.from_numpy(truth).to(dev()), affines[1], P.GeometrySpec('RAS', 'vote', reg))
    _, found = coreg.coregister_case(vols, affines, **reg)
    assert r['follows'] == 1 == P.truth_follows([fs, ms], affines, ms, affines[1])
    assert r['coreg'][0] is None and r['coreg'][1].params == found[1].params
    print('registration: %s' % coreg.format_result('moving', found[1]))
    assert found[1].nmi_after >= found[1].nmi_before
    assert np.array_equal(r['affines'][0], affines[0]) and np.array_equal(r['affines'][1], found[1].affine)
    assert np.array_equal(r['truth_affine'], np.linalg.inv(found[1].matrix) @ affines[1])      # the same correction
    assert np.array_equal(r['truth_affine'], r['affines'][1])
    assert r['label_path'] == 'vote' and np.array_equal(r['truth_matrix'], r['plan']['matrices'][1])
    shape = r['plan']['shape']
    ref, margin = labelvote_ref.label_vote(truth, r['truth_matrix'], shape)
    sure = (margin >= 1e-9) & ~conform_ref.near_a_decision(r['truth_matrix'], shape, ms, 1, eps=1e-6)
    assert sure.mean() > 0.99
    assert tuple(r['y'].shape) == tuple(shape) + (1,) and np.array_equal(r['y'][..., 0].cpu().numpy()[sure], ref[sure])
    # a truth on the first modality's grid is not moved
    first = labelvote_ref.label_volume(fs, 42)
    assert P.truth_follows([fs, ms], affines, fs, affines[0]) == 0
    plain = P.conform_case(vols, affines, torch.from_numpy(first).to(dev()), affines[0], P.GeometrySpec('RAS', 'vote', None))
    assert plain['coreg'] is None and plain['label_path'] == 'reorient' and np.array_equal(plain['y'][..., 0].cpu().numpy(), first)
