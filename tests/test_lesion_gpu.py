"""GPU: the kernels of csrc/lesion.hip, their wrappers, bts_amd.infer.lesionwise_scores and the --lesionwise flag of `python -m
bts_amd.test` against the SciPy restatement (tests/lesion_ref.py).  Everything that is an integer is compared with array_equal; the
final scores within 1e-12 relative, the bound tests/test_surface_gpu.py holds for the same percentile arithmetic.  Shapes: an extent of
1, lines shorter and longer than a wave, extents that are no multiple of the 64 x 8 x 8 labelling tile or of the dilation tile (at most
64 x 16 x 16, less twice the iterations of a pass), sets on every face of the volume."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lesion_ref as L  # noqa: E402
import segment_ref as S  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

SHAPES = [(1, 9, 70), (3, 5, 130), (9, 17, 70), (24, 40, 72)]
SENTINEL = 7
REL = 1e-12


def dev():
    return torch.device('cuda', 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def ops():
    import bts_amd  # noqa: F401
    from bts_amd import ops as o
    return o


def labels(shape, density, seed):
    """labels {1, 2, 4} on a `density` share of the voxels, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    lab = np.array([1, 2, 4], dtype=np.uint8)[rng.integers(0, 3, size=shape)]
    lab[rng.random(shape) >= density] = 0
    return lab


def close(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= REL * max(abs(a), abs(b))


# ---- dilate3d ----------------------------------------------------------------------------------------------------------------------------
def dilate_inputs(shape):
    corner = np.zeros(shape, np.uint8)
    corner[-1, -1, -1] = 4
    first = np.zeros(shape, np.uint8)
    first[0, 0, 0] = 1
    return {'seeds': labels(shape, 0.02, 11), 'full': np.full(shape, 2, np.uint8), 'empty': np.zeros(shape, np.uint8), 'last_corner': corner,
            'first_corner': first}


@pytest.mark.parametrize('iterations', [0, 1, 3])
@pytest.mark.parametrize('conn', [6, 18, 26])
@pytest.mark.parametrize('shape', SHAPES)
def test_dilation_equals_scipy(shape, conn, iterations):
    o = ops()
    for name, lab in dilate_inputs(shape).items():
        for cm in (14, 8):
            want = L.dilate(L.region(lab, cm), conn, iterations).astype(np.uint8)
            got = o.dilate3d(gpu(lab), cm, 4, conn, iterations)
            assert got.dtype == torch.uint8 and tuple(got.shape) == shape
            assert np.array_equal(got.cpu().numpy(), want), (name, cm)


@pytest.mark.parametrize('iterations,fuse', [(3, 1), (3, 2), (7, 0), (7, 6), (5, 4), (2, 5)])
@pytest.mark.parametrize('shape', [(9, 17, 70), (24, 40, 72)])
def test_dilation_in_passes_of_every_size(shape, iterations, fuse):
    """several passes through the workspace, an odd and an even number of them, and a pass wider than the default"""
    o = ops()
    lab = labels(shape, 0.003, 5)
    lab[0, 0, 0] = lab[-1, -1, -1] = 1
    for conn in (6, 18, 26):
        want = L.dilate(L.region(lab, 14), conn, iterations).astype(np.uint8)
        got = o.dilate3d(gpu(lab), 14, 4, conn, iterations, fuse=fuse)
        assert np.array_equal(got.cpu().numpy(), want), conn
        assert 0 < int(want.sum()) < want.size or iterations >= 7                     # the case tells a wrong halo from a right one


@pytest.mark.parametrize('off', [1, 3])
def test_dilation_out_argument_and_unaligned_views(off):
    o = ops()
    shape = (9, 17, 70)
    lab = labels(shape, 0.02, 3)
    n = lab.size
    want = L.dilate(L.region(lab, 14), 18, 3).astype(np.uint8)
    store = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device=dev())
    src = store[off:off + n].view(shape)
    src.copy_(gpu(lab))
    dst_store = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device=dev())
    dst = dst_store[off:off + n].view(shape)
    got = o.dilate3d(src, 14, 4, 18, 3, out=dst)
    assert got.data_ptr() == dst.data_ptr() and np.array_equal(dst.cpu().numpy(), want)
    edge = dst_store.cpu().numpy()
    assert (edge[:off] == SENTINEL).all() and (edge[off + n:] == SENTINEL).all()      # nothing outside the map is written
    assert np.array_equal(src.cpu().numpy(), lab)
    again = o.dilate3d(src, 14, 4, 18, 3, fuse=1, out=dst)
    assert np.array_equal(again.cpu().numpy(), want)


def test_wrappers_refuse_what_the_entry_points_refuse():
    o = ops()
    lab = gpu(labels((4, 5, 6), 0.5, 1))
    comp = torch.zeros((4, 5, 6), dtype=torch.int32, device=dev())
    with pytest.raises(ValueError):
        o.dilate3d(lab.view(-1), 14)
    with pytest.raises(ValueError):
        o.dilate3d(lab, 14, out=lab)
    with pytest.raises(ValueError):
        o.dilate3d(lab, 14, out=torch.zeros(5, dtype=torch.uint8, device=dev()))
    with pytest.raises(ValueError):
        o.dilate3d(lab.cpu(), 14)
    for kw in (dict(connectivity=8), dict(iterations=-1), dict(fuse=7), dict(K=9), dict(class_mask=16)):
        args = dict(class_mask=14)
        args.update(kw)
        with pytest.raises(RuntimeError):
            o.dilate3d(lab, **args)
    with pytest.raises(ValueError):
        o.lesion_pairs(comp, lab, comp.view(-1)[:5], 14)
    with pytest.raises(ValueError):
        o.lesion_pairs(comp, lab, comp, 14, capacity=0)
    with pytest.raises(ValueError):
        o.lesion_pairs(comp.long(), lab, comp, 14)
    with pytest.raises(ValueError):
        o.component_boxes(comp, [5, 3])
    with pytest.raises(ValueError):
        o.component_boxes(comp.view(-1), [3])
    for box in ((0, 0, 0, 5, 5, 6), (2, 0, 0, 2, 5, 6), (-1, 0, 0, 4, 5, 6), (0, 0, 0, 4, 5)):
        with pytest.raises(ValueError):
            o.lesion_crop(comp, lab, comp, 14, box, 0, [])
    with pytest.raises(ValueError):
        o.lesion_crop(comp, lab, comp, 14, (0, 0, 0, 4, 5, 6), 0, [], out=(lab, lab.view(-1)[:7]))
    with pytest.raises(RuntimeError):
        o.lesion_crop(comp, lab, comp, 14, (0, 0, 0, 4, 5, 6), 120, [])


# ---- lesion_pairs, component_boxes ------------------------------------------------------------------------------------------------------
def noise_case(shape, dilation):
    """5 % noise in truth and prediction -> the restatement's maps and answers"""
    truth, pred = labels(shape, 0.05, 21), labels(shape, 0.05, 22)
    t = L.region(truth, 14)
    td = L.components(L.dilate(t, 18, dilation), 26)
    pc = L.components(L.region(pred, 14), 26)
    rows, vox = L.pairs(td, t, pc)
    return truth, td, pc, rows, vox


@pytest.mark.parametrize('dilation', [0, 1])
@pytest.mark.parametrize('shape', SHAPES)
def test_pairs_equal_the_restatement(shape, dilation):
    o = ops()
    truth, td, pc, rows, vox = noise_case(shape, dilation)
    if shape == SHAPES[-1]:
        assert len(rows) >= 100 and len(L.roots_of(pc)) >= 100                        # hundreds of components and pairs
    got, gvox = o.lesion_pairs(gpu(td), gpu(truth), gpu(pc), 14)
    assert got.dtype == np.int64 and np.array_equal(got, rows)
    assert gvox.dtype == torch.int32 and np.array_equal(gvox.cpu().numpy(), vox)
    # a table of one slot: the grow path, the same rows
    small, svox = o.lesion_pairs(gpu(td), gpu(truth), gpu(pc), 14, capacity=1)
    assert np.array_equal(small, rows) and torch.equal(svox, gvox)
    # given counts, a given buffer pre-filled with a sentinel, and a second run: the same bytes
    buf = torch.full((td.size,), SENTINEL, dtype=torch.int32, device=dev())
    again, avox = o.lesion_pairs(gpu(td), gpu(truth), gpu(pc), 14, counts=(len(L.roots_of(td)), len(L.roots_of(pc))), lesion_vox=buf)
    assert avox.data_ptr() == buf.data_ptr() and again.tobytes() == got.tobytes() and torch.equal(avox, gvox)
    # another region of the same truth map
    t8 = L.region(truth, 8)
    rows8, vox8 = L.pairs(td, t8 & (td > 0), pc)
    got8, gvox8 = o.lesion_pairs(gpu(td), gpu(truth), gpu(pc), 8)
    assert np.array_equal(got8, rows8) and np.array_equal(gvox8.cpu().numpy(), vox8)


def test_pairs_off_a_16_byte_boundary_and_empty_maps():
    o = ops()
    shape = (9, 17, 70)
    truth, td, pc, rows, vox = noise_case(shape, 1)
    n = td.size
    a = torch.zeros(n + 4, dtype=torch.int32, device=dev())
    b = torch.zeros(n + 4, dtype=torch.int32, device=dev())
    a[1:n + 1].copy_(gpu(td).view(-1))
    b[3:n + 3].copy_(gpu(pc).view(-1))
    t = torch.zeros(n + 4, dtype=torch.uint8, device=dev())
    t[1:n + 1].copy_(gpu(truth).view(-1))
    got, gvox = o.lesion_pairs(a[1:n + 1], t[1:n + 1], b[3:n + 3], 14)
    assert np.array_equal(got, rows) and np.array_equal(gvox.cpu().numpy(), vox)
    zero = torch.zeros(shape, dtype=torch.int32, device=dev())
    got, gvox = o.lesion_pairs(zero, gpu(truth), gpu(pc), 14)
    assert got.shape == (0, 4) and int(gvox.abs().sum()) == 0
    got, gvox = o.lesion_pairs(gpu(td), gpu(truth), zero, 14)
    assert got.shape == (0, 4) and np.array_equal(gvox.cpu().numpy(), vox)


@pytest.mark.parametrize('shape', SHAPES)
def test_boxes_equal_the_restatement(shape):
    o = ops()
    _, td, pc, _, _ = noise_case(shape, 1)
    for comp in (td, pc):
        roots = L.roots_of(comp)
        want = L.boxes(comp, roots)
        got = o.component_boxes(gpu(comp), gpu(roots.astype(np.int32)))
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        some = roots[::3]
        out = torch.full((len(some), 6), SENTINEL, dtype=torch.int32, device=dev())
        got = o.component_boxes(gpu(comp), [int(r) for r in some], out=out)
        assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want[::3])
        assert torch.equal(o.component_boxes(gpu(comp), [int(r) for r in some]), out)  # two runs, the same bytes
    assert tuple(o.component_boxes(gpu(pc), []).shape) == (0, 6)
    # a root the map does not hold keeps the empty box
    absent = next(v for v in range(pc.size) if pc.reshape(-1)[v] != v + 1)
    got = o.component_boxes(gpu(pc), [absent]).cpu().numpy()
    assert got.tolist() == [[2 ** 31 - 1] * 3 + [0] * 3]


def test_boxes_of_sets_on_every_face():
    o = ops()
    shape = (24, 40, 72)
    full = np.ones(shape, np.uint8)
    comp = L.components(full, 6)
    assert o.component_boxes(gpu(comp), [0]).cpu().numpy().tolist() == [[0, 0, 0, 24, 40, 72]]
    t, p = L.multi_lesion_pair()
    pc = L.components(L.region(p, 14), 26)
    roots = L.roots_of(pc)
    assert np.array_equal(o.component_boxes(gpu(pc), roots.tolist()).cpu().numpy(), L.boxes(pc, roots))


# ---- lesion_crop -------------------------------------------------------------------------------------------------------------------------
def test_crops_equal_the_restatement():
    o = ops()
    truth, pred = L.multi_lesion_pair()
    shape = truth.shape
    for cm in (14, 10, 8):
        t = L.region(truth, cm)
        td = L.components(L.dilate(t, 18, 3), 26)
        pc = L.components(L.region(pred, cm), 26)
        rows, _ = L.pairs(td, t, pc)
        tdb = dict(zip(L.roots_of(td).tolist(), L.boxes(td, L.roots_of(td))))
        pcb = dict(zip(L.roots_of(pc).tolist(), L.boxes(pc, L.roots_of(pc))))
        corners = 0
        for root in L.roots_of(td).tolist():
            comps = [int(c) for c in rows[rows[:, 0] == root][:, 1]]
            bs = np.stack([tdb[root]] + [pcb[c] for c in comps])
            box = tuple(bs[:, :3].min(axis=0).tolist()) + tuple(bs[:, 3:].max(axis=0).tolist())
            corners += box[:3] == (0, 0, 0) or box[3:] == shape
            g_ref, m_ref = L.crop(td, t, pc, box, root, comps)
            g, m = o.lesion_crop(gpu(td), gpu(truth), gpu(pc), cm, box, root, comps)
            assert g.dtype == torch.uint8 and tuple(g.shape) == g_ref.shape == tuple(m.shape)
            assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(m.cpu().numpy(), m_ref), (cm, root)
            # the restatement's own claim: the box holds all of the lesion and of its components
            assert int(g_ref.sum()) == int((t & (td == root + 1)).sum()) and int(m_ref.sum()) == int(np.isin(pc, np.array(comps) + 1).sum())
        assert corners >= 1, cm                                                       # a box at a corner of the volume
    # the whole volume as the box, given buffers off a 4-byte boundary, roots as a tensor
    t = L.region(truth, 14)
    td = L.components(L.dilate(t, 18, 3), 26)
    pc = L.components(L.region(pred, 14), 26)
    root, comps = int(L.roots_of(td)[0]), L.roots_of(pc)[:2]
    box = (0, 0, 0) + shape
    g_ref, m_ref = L.crop(td, t, pc, box, root, comps)
    store = torch.full((2, truth.size + 4), SENTINEL, dtype=torch.uint8, device=dev())
    out = (store[0, 1:truth.size + 1], store[1, 3:truth.size + 3])
    g, m = o.lesion_crop(gpu(td), gpu(truth), gpu(pc), 14, box, root, gpu(comps.astype(np.int32)), out=out)
    assert np.array_equal(g.cpu().numpy().reshape(shape), g_ref) and np.array_equal(m.cpu().numpy().reshape(shape), m_ref)
    edge = store.cpu().numpy()
    assert (edge[0, :1] == SENTINEL).all() and (edge[0, -3:] == SENTINEL).all() and (edge[1, :3] == SENTINEL).all() and edge[1, -1] == SENTINEL


# ---- lesionwise_scores ---------------------------------------------------------------------------------------------------------------------
def assert_same_scores(got, want, names):
    for name in names:
        assert got['lw_counts_' + name] == want['lw_counts_' + name], name
        rows, ref = got['lw_lesions_' + name], want['lw_lesions_' + name]
        assert len(rows) == len(ref), name
        for i, (a, b) in enumerate(zip(rows, ref)):
            assert set(a) == set(b) == {'voxels', 'matched_components', 'matched_voxels', 'overlap', 'dice', 'hd95'}
            for key in ('voxels', 'matched_components', 'matched_voxels', 'overlap'):
                assert a[key] == b[key] and isinstance(a[key], int), (name, i, key)
            assert a['dice'] == b['dice'], (name, i)                                  # one float64 division of the same integers
            print('%s lesion %d: hd95 %.17g, restatement %.17g' % (name, i, a['hd95'], b['hd95']))
            assert close(a['hd95'], b['hd95']), (name, i, a['hd95'], b['hd95'])
        for key in ('lw_dice_', 'lw_hd95_'):
            print('%s%s: %.17g, restatement %.17g' % (key, name, got[key + name], want[key + name]))
            assert close(got[key + name], want[key + name]), (key, name, got[key + name], want[key + name])


@pytest.mark.parametrize('name', sorted(L.known_cases()))
def test_scores_of_the_known_answers(name):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    t, p, kw, (dice, hd, counts) = L.known_cases()[name]
    truth, pred = t.astype(np.uint8) * 2, p.astype(np.uint8) * 2
    got = infer.lesionwise_scores(gpu(truth), gpu(pred), (1.0, 1.0, 1.0), regions=(('x', (1, 2, 3)),), **kw)
    assert set(got) == {'lw_dice_x', 'lw_hd95_x', 'lw_counts_x', 'lw_lesions_x'}
    assert close(got['lw_dice_x'], dice) and got['lw_counts_x'] == counts
    if hd is not None:
        assert close(got['lw_hd95_x'], hd)
    assert_same_scores(got, L.lesionwise_scores(truth, pred, (1.0, 1.0, 1.0), regions=(('x', (1, 2, 3)),), **kw), ['x'])


@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (1.2, 1.0, 0.9)])
def test_scores_of_the_multi_lesion_pair(spacing):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    truth, pred = L.multi_lesion_pair()
    want = L.lesionwise_scores(truth, pred, spacing)
    assert want['lw_counts_wt'] == {'lesions': 5, 'false_negatives': 1, 'false_positives': 1, 'ignored': 1}     # the case is what it says
    got = infer.lesionwise_scores(gpu(truth), gpu(pred), spacing)
    assert set(got) == set(want)
    assert_same_scores(got, want, ['wt', 'tc', 'et'])
    again = infer.lesionwise_scores(truth, pred, spacing)                             # numpy in, and a second run: the same numbers
    assert repr(again) == repr(got)
    # other parameters, two classes
    kw = dict(dilation=1, dilation_connectivity=26, connectivity=6, min_lesion_voxels=0, penalty_mm=100.0, percentile=50.0)
    t2, p2 = np.minimum(truth, 1), np.minimum(pred, 1)
    got = infer.lesionwise_scores(gpu(t2), gpu(p2), spacing, n_classes=2, **kw)
    assert_same_scores(got, L.lesionwise_scores(t2, p2, spacing, n_classes=2, **kw), ['class_1'])


def test_scores_of_noise():
    """hundreds of lesions and components, most of them ignored at 5 voxels; the pairs, the order and the sums still agree"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    shape = (9, 17, 70)
    truth, pred = labels(shape, 0.08, 31), labels(shape, 0.08, 32)
    kw = dict(dilation=0, min_lesion_voxels=3)
    want = L.lesionwise_scores(truth, pred, (1.0, 1.0, 1.0), **kw)
    assert want['lw_counts_wt']['lesions'] >= 5 and want['lw_counts_wt']['ignored'] >= 20 and want['lw_counts_wt']['false_positives'] >= 20
    assert_same_scores(infer.lesionwise_scores(gpu(truth), gpu(pred), (1.0, 1.0, 1.0), **kw), want, ['wt', 'tc', 'et'])


def test_scores_refuse_bad_arguments():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    lab = gpu(labels((4, 5, 6), 0.5, 1))
    for kw in (dict(percentile=101.0), dict(dilation=-1), dict(min_lesion_voxels=-1), dict(penalty_mm=-1.0)):
        with pytest.raises(ValueError):
            infer.lesionwise_scores(lab, lab, (1.0, 1.0, 1.0), **kw)
    with pytest.raises(ValueError):
        infer.lesionwise_scores(lab, lab[:3], (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        infer.lesionwise_scores(lab, lab, (1.0, 1.0))


# ---- the command -------------------------------------------------------------------------------------------------------------------
SKULL_KW = dict(base_filters=4, groups=2, reduction=2, depth=2, out_ch=1)
TUMOR_KW = dict(base_filters=8, groups=2, reduction=2, depth=3)
VOL, SEED = (11, 9, 14), 5
SKULL_STATS = ([95.0, 110.0], [35.0, 45.0])
TUMOR_STATS = ([60.0, 70.0], [30.0, 40.0])


def write_case(folder, vol, seed, affine):
    """the labelled fixture case of tests/test_components_gpu.py"""
    from bts_amd import nifti
    os.makedirs(folder)
    x = S.scan_like(vol, seed)
    nifti.save(os.path.join(folder, 'c_t1ce.nii.gz'), x[..., 0], affine)
    nifti.save(os.path.join(folder, 'c_flair.nii'), x[..., 1], affine)
    y = np.array([0, 1, 2, 4], dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=vol)]
    nifti.save(os.path.join(folder, 'c_seg.nii.gz'), y.astype(np.int16), affine)
    return y


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


def read(path, mode='rb'):
    with open(path, mode) as f:
        return f.read()


def test_command_with_and_without_the_flag(tmp_path, capsys):
    """three labelled cases (one with non-unit pixdim), two checkpoints.  Without the flag: the file label_scores gives by hand, and the
    flagged file less its last fifteen columns.  With it: every row and the total recomputed by the restatement from the written
    mask.nii and the truth; --workers 0 against --workers 2; after the columns of --surface_metrics when both are on."""
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti
    from bts_amd import test as T
    data = tmp_path / 'data'
    affines = {'a': np.eye(4), 'b': np.diag([1.2, 1.0, 0.9, 1.0]), 'c': np.eye(4)}
    pixdims = {'a': (1.0, 1.0, 1.0), 'b': (1.2, 1.0, 0.9), 'c': (1.0, 1.0, 1.0)}
    truth = {name: write_case(str(data / name), VOL, 5 + i, affines[name]) for i, name in enumerate('abc')}
    write_model(str(tmp_path / 'tumor'), TUMOR_KW, (32, 16, 16), True, SEED + 20)
    write_model(str(tmp_path / 'skull'), SKULL_KW, S.padded(VOL, 4), False, SEED + 10)
    for name, (mean, std) in (('tp.npy', TUMOR_STATS), ('sp.npy', SKULL_STATS)):
        np.save(str(tmp_path / name), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                       'norm': {'mean': np.array(mean).reshape(1, 1, 1, 2), 'std': np.array(std).reshape(1, 1, 1, 2)}})
    base = ['--in_locs', str(data), '--modalities', 't1ce,flair', '--truth', 'seg', '--gpu',
            '--tumor_model', str(tmp_path / 'tumor'), '--tumor_prepro', str(tmp_path / 'tp.npy'),
            '--skull_model', str(tmp_path / 'skull'), '--skull_prepro', str(tmp_path / 'sp.npy')]
    head = ['case', 'macro', 'micro', 'dice_1', 'dice_2', 'dice_3', 'wt', 'tc', 'et']

    plain = tmp_path / 'plain'
    T.run(T.parse_args(base + ['--workers', '0', '--out_loc', str(plain)]))
    assert 'Lesion-wise' not in capsys.readouterr().out
    masks = {name: nifti.load(str(plain / name / 'mask.nii'))[0] for name in 'abc'}
    conf = np.zeros((4, 4), dtype=np.int64)
    rows = [head]
    for name in 'abc':
        s = infer.label_scores(truth[name], masks[name], 4)
        rows.append(T.score_row(name, s))
        conf += s['confusion']
    rows.append(T.score_row('total', infer.scores_from_confusion(conf)))
    plain_text = read(str(plain / 'scores.csv'), 'r')
    assert plain_text == ''.join(','.join(r) + '\n' for r in rows)                     # the file the command has always written

    def widened(name):
        return tuple(float(np.float32(v)) for v in pixdims[name])

    def expected(kw):
        cols = {name: T.lesion_columns(L.lesionwise_scores(truth[name], masks[name], widened(name), **kw)) for name in 'abc'}
        total = {k: T.mean_finite([cols[n][k] for n in 'abc']) for k in T.LESION_SCORE_KEYS}
        total.update({k: sum(cols[n][k] for n in 'abc') for k in T.LESION_COUNT_KEYS})
        return [list(T.LESION_KEYS)] + [T.lesion_row(cols[n]) for n in 'abc'] + [T.lesion_row(total)], cols

    flags = ['--lesionwise', '--lesion_dilation', '1', '--lesion_min_voxels', '5', '--lesion_penalty_mm', '100']
    want, cols = expected(dict(dilation=1, min_lesion_voxels=5, penalty_mm=100.0))
    assert sum(cols[n]['lw_lesions_wt'] for n in 'abc') >= 3                          # the fixtures give the score something to do
    outs = []
    for workers in (0, 2):
        out = tmp_path / ('flag%d' % workers)
        res = T.run(T.parse_args(base + flags + ['--workers', str(workers), '--out_loc', str(out)]))
        assert res['scored'] == 3
        outs.append(out)
    assert capsys.readouterr().out.count('. Lesion-wise Dice WT: ') == 6
    text = read(str(outs[0] / 'scores.csv'), 'r')
    assert text == read(str(outs[1] / 'scores.csv'), 'r')
    for name in 'abc':
        assert read(str(outs[0] / name / 'mask.nii')) == read(str(outs[1] / name / 'mask.nii')) == read(str(plain / name / 'mask.nii'))
    got = [line.split(',') for line in text.splitlines()]
    assert [','.join(r[:-15]) + '\n' for r in got] == plain_text.splitlines(keepends=True)
    for r, w in zip(got, want):
        print(r[0], r[-15:], w)
        assert r[-15:] == w, r[0]
    assert len(got) == len(want) == 5

    # defaults, with --surface_metrics: the lesion-wise columns come last
    both = tmp_path / 'both'
    T.run(T.parse_args(base + ['--lesionwise', '--surface_metrics', '--workers', '0', '--out_loc', str(both)]))
    capsys.readouterr()
    want, _ = expected({})
    got = [line.split(',') for line in read(str(both / 'scores.csv'), 'r').splitlines()]
    assert got[0] == head + list(T.SURFACE_KEYS) + list(T.LESION_KEYS)
    assert [','.join(r[:9]) + '\n' for r in got] == plain_text.splitlines(keepends=True)
    assert [r[-15:] for r in got] == want
