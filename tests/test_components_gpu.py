"""-m gpu: csrc/components.hip (bts_components3d, bts_component_sizes, bts_component_largest, bts_components_apply, bts_region_relabel)
against the NumPy restatement of tests/components_ref.py, everything with array_equal: there are no tolerances.  Then
infer.remove_components / postprocess_labels, the largest-component option of the skull stage of infer.segment_case, and `python -m
bts_amd.test` with the post-processing flags on three tiny cases.

Shapes: a line shorter than a wave (5,6,7), an extent of 1 (1,9,70), a row longer than a workgroup (17,3,300), several tiles on every
axis (33,70,65), and the tile extent (8,8,64) plus one on every axis (9,9,65): every kind of seam is crossed by exactly one voxel."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import components_ref as C  # noqa: E402
import segment_ref as S  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

TILE = (8, 8, 64)
SHAPES = [(5, 6, 7), (1, 9, 70), (17, 3, 300), (33, 70, 65), tuple(t + 1 for t in TILE)]
SENTINEL = -7


def dev():
    return torch.device('cuda', 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def inputs(shape):
    last = np.zeros(shape, np.uint8)
    last[-1, -1, -1] = 4
    return {'random50': C.random_labels(shape, 0.5, 1), 'random05': C.random_labels(shape, 0.05, 2), 'checkerboard': C.checkerboard(shape),
            'serpentine': C.serpentine(shape), 'full': np.full(shape, 2, np.uint8), 'empty': np.zeros(shape, np.uint8), 'last': last}


def label(lab, cm, k, conn, **kw):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops.components3d(lab if isinstance(lab, torch.Tensor) else gpu(lab), cm, k, conn, **kw)


# ---- bts_components3d ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conn', [6, 18, 26])
@pytest.mark.parametrize('shape', SHAPES)
def test_labelling_equals_the_restatement(shape, conn):
    """comp starts as a sentinel (every element must be written), and a second run gives the same bytes"""
    n = int(np.prod(shape))
    for name, lab in inputs(shape).items():
        ref = C.components3d(lab, 14, 4, conn)
        out = torch.full(shape, SENTINEL, dtype=torch.int32, device=dev())
        got = label(lab, 14, 4, conn, out=out)
        assert got is out and got.dtype == torch.int32
        g = got.cpu().numpy()
        assert np.array_equal(g, ref), (name, int((g != ref).sum()))
        again = label(lab, 14, 4, conn).cpu().numpy()
        assert again.tobytes() == g.tobytes(), name
        ncomp = C.sizes(ref)[1]
        if name == 'checkerboard':
            assert ncomp == (int(lab.sum()) if conn == 6 else 1)
        elif name in ('serpentine', 'full'):
            assert ncomp == 1 and g.max() == 1
        elif name == 'empty':
            assert ncomp == 0 and not g.any()
        elif name == 'last':
            assert ncomp == 1 and g.reshape(-1)[-1] == n and int((g != 0).sum()) == 1


def test_pairs_across_a_tile_seam_tell_the_connectivities_apart():
    """the eight voxels around the corner where eight tiles meet: every pair of them (12 share a face, 12 only an edge, 4 only a corner),
    alone in the volume, is one component or two by the connectivity alone"""
    shape = SHAPES[-1]
    cube = [(TILE[0] - 1 + a, TILE[1] - 1 + b, TILE[2] - 1 + c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    seen = {1: 0, 2: 0, 3: 0}
    for i, p in enumerate(cube):
        for q in cube[i + 1:]:
            dist = sum(abs(u - v) for u, v in zip(p, q))
            seen[dist] += 1
            lab = np.zeros(shape, np.uint8)
            lab[p] = lab[q] = 1
            for conn, reach in ((6, 1), (18, 2), (26, 3)):
                g = label(lab, 2, 2, conn).cpu().numpy()
                assert np.array_equal(g, C.components3d(lab, 2, 2, conn)), (p, q, conn)
                assert len(np.unique(g[g > 0])) == (1 if dist <= reach else 2), (p, q, conn)
    assert seen == {1: 12, 2: 12, 3: 4}


@pytest.mark.parametrize('k,masks', [(2, (2, 1)), (4, (14, 10, 8, 1, 5)), (8, (0b10010110, 128, 1))])
def test_class_counts_and_class_masks(k, masks):
    """labels 3 and 7 join the set so that K = 8 tells them apart; the masks with bit 0 select the background"""
    for shape, conn in (((33, 70, 65), 26), ((17, 3, 300), 6)):
        rng = np.random.default_rng(k)
        lab = np.array([0, 0, 0, 1, 2, 3, 4, 7, 255], np.uint8)[rng.integers(0, 9, size=shape)]
        for cm in masks:
            ref = C.components3d(lab, cm, k, conn)
            assert ref.any()
            assert np.array_equal(label(lab, cm, k, conn).cpu().numpy(), ref), (shape, cm)


@pytest.mark.parametrize('off', [1, 3])
def test_label_map_off_a_4_byte_boundary(off):
    shape = (17, 3, 300)
    n = int(np.prod(shape))
    lab = C.random_labels(shape, 0.5, 7)
    buf = torch.zeros(n + 8, dtype=torch.uint8, device=dev())
    assert buf.data_ptr() % 4 == 0
    view = buf[off:off + n].view(shape)
    view.copy_(gpu(lab))
    assert view.data_ptr() % 4 == off and view.is_contiguous()
    assert np.array_equal(label(view, 14, 4, 18).cpu().numpy(), C.components3d(lab, 14, 4, 18))


def test_wrappers_refuse_what_the_entry_points_refuse():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    lab = torch.zeros((4, 5, 6), dtype=torch.uint8, device=dev())
    for kw in (dict(class_mask=16), dict(class_mask=14, K=9), dict(class_mask=14, connectivity=8)):
        with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
            ops.components3d(lab, **kw)
    with pytest.raises(ValueError, match='uint8'):
        ops.components3d(lab.int(), 14)
    with pytest.raises(ValueError, match='D,H,W'):
        ops.components3d(lab.view(-1), 14)
    with pytest.raises(ValueError, match='int32'):
        ops.components3d(lab, 14, out=torch.zeros((4, 5, 6), device=dev()))


# ---- sizes, key, apply ---------------------------------------------------------------------------------------------------------------
def planted():
    """two components of 5 voxels (the second across a tile seam) and one of 3, in labels of class 3 (4 and 255 mixed) among voxels of
    labels 0, 1 and 2 that the region (class mask 8) leaves out: whatever is stored where it should not be shows"""
    shape = SHAPES[-1]
    lab = np.array([0, 1, 2], np.uint8)[np.random.default_rng(3).integers(0, 3, size=shape)]
    lab[0, 0, 10:15] = [4, 255, 4, 255, 4]
    lab[8, 8, 60:65] = [255, 4, 4, 4, 255]
    lab[4, 4, 30:33] = 4
    return lab


def check_sizes_key_apply(lab, cm, k, conn, min_voxels, largest_only, fill):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    n = lab.size
    comp_ref = C.components3d(lab, cm, k, conn)
    size_ref, found = C.sizes(comp_ref)
    comp = label(lab, cm, k, conn)
    size = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev())               # the call zeroes it
    count = torch.zeros(1, dtype=torch.int64, device=dev())
    got_size, got_count = ops.component_sizes(comp, out=size, count=count)
    assert got_size is size and got_count is count
    assert np.array_equal(size.cpu().numpy(), size_ref) and int(count.item()) == found
    ops.component_sizes(comp, out=size, count=count)                                 # the sizes again, the count accumulated
    assert np.array_equal(size.cpu().numpy(), size_ref) and int(count.item()) == 2 * found
    key = torch.full((1,), SENTINEL, dtype=torch.int64, device=dev())                # ... and zeroes this
    assert ops.component_largest(size, out=key) is key
    assert int(key.item()) == C.largest_key(size_ref)
    want, vox, gone = C.apply(lab, comp_ref, size_ref, min_voxels, largest_only, fill)
    removed = torch.zeros(2, dtype=torch.int64, device=dev())
    for calls in (1, 2):                                                             # each on a fresh copy, the counters accumulated
        work = gpu(lab)
        assert ops.components_apply(work, comp, size, key if largest_only else None, min_voxels, largest_only, fill, removed=removed) is removed
        got = work.cpu().numpy()
        assert np.array_equal(got, want)
        untouched = (comp_ref == 0) | (want == lab)
        assert np.array_equal(got[untouched], lab[untouched])
        assert removed.cpu().tolist() == [calls * vox, calls * gone]
    return vox, gone


@pytest.mark.parametrize('fill', [0, 1])
def test_sizes_key_and_apply_on_the_planted_components(fill):
    lab = planted()
    size = C.sizes(C.components3d(lab, 8, 4, 26))[0]
    assert size[10] == 5 and size[(8 * 9 + 8) * 65 + 60] == 5 and size[(4 * 9 + 4) * 65 + 30] == 3 and int((size > 0).sum()) == 3
    assert C.key_root(C.largest_key(size)) == 10                                     # of the equal pair, the one that starts first
    assert check_sizes_key_apply(lab, 8, 4, 26, 0, True, fill) == (8, 2)
    assert check_sizes_key_apply(lab, 8, 4, 26, 4, False, fill) == (3, 1)            # size - 1 of the fives: they stay
    assert check_sizes_key_apply(lab, 8, 4, 26, 5, False, fill) == (3, 1)            # size: they stay
    assert check_sizes_key_apply(lab, 8, 4, 26, 6, False, fill) == (13, 3)           # size + 1: they go
    assert check_sizes_key_apply(lab, 8, 4, 26, 3, False, fill) == (0, 0)
    assert check_sizes_key_apply(lab, 8, 4, 26, 4, True, fill) == (8, 2)


@pytest.mark.parametrize('shape,conn', [((33, 70, 65), 6), ((33, 70, 65), 26), ((17, 3, 300), 18), ((1, 9, 70), 26), ((5, 6, 7), 6)])
def test_sizes_key_and_apply_on_random_maps(shape, conn):
    """50 % density: thousands of components under 6 neighbours, one that holds nearly everything under 26 (the workgroup's key
    component in the sizes kernel); the empty map: no component, key 0, nothing written"""
    lab = C.random_labels(shape, 0.5, 5)
    check_sizes_key_apply(lab, 14, 4, conn, 3, False, 0)
    check_sizes_key_apply(lab, 14, 4, conn, 0, True, 1)
    check_sizes_key_apply(np.full(shape, 1, np.uint8), 14, 4, conn, 2, True, 0)
    assert check_sizes_key_apply(np.zeros(shape, np.uint8), 14, 4, conn, 2, True, 9) == (0, 0)


def test_remove_components_and_postprocess_labels_equal_the_restatement():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    shape = (33, 70, 65)
    lab = C.random_labels(shape, 0.2, 9)
    lab[lab == 255] = 4
    for kw in (dict(min_voxels=4), dict(largest_only=True), dict(min_voxels=3, largest_only=True, fill=1, connectivity=6)):
        want, counts = C.remove_components(lab, 14, 4, **kw)
        work = gpu(lab)
        assert infer.remove_components(work, 14, 4, **kw) == counts
        assert np.array_equal(work.cpu().numpy(), want)
    n_et = int((lab == 4).sum())
    for kw in (dict(min_component_voxels=5), dict(et_min_voxels=n_et + 1), dict(et_min_voxels=n_et),
               dict(min_component_voxels=3, et_min_voxels=n_et, connectivity=6), dict()):
        want, counts = C.postprocess_labels(lab, **kw)
        work = gpu(lab)
        assert infer.postprocess_labels(work, **kw) == counts, kw
        assert np.array_equal(work.cpu().numpy(), want), kw
    assert C.postprocess_labels(lab, et_min_voxels=n_et + 1)[1]['et_relabelled'] == n_et
    assert C.postprocess_labels(lab, et_min_voxels=n_et)[1]['et_relabelled'] == 0
    assert C.postprocess_labels(lab, min_component_voxels=3, et_min_voxels=n_et, connectivity=6)[1]['et_relabelled'] > 0
    with pytest.raises(ValueError, match='negative'):
        infer.postprocess_labels(gpu(lab), min_component_voxels=-1)


# ---- the two-stage path ------------------------------------------------------------------------------------------------------------------
SKULL_KW = dict(base_filters=4, groups=2, reduction=2, depth=2, out_ch=1)
TUMOR_KW = dict(base_filters=8, groups=2, reduction=2, depth=3)
VOL, SEED = (11, 9, 14), 5
SKULL_STATS = ([95.0, 110.0], [35.0, 45.0])
TUMOR_STATS = ([60.0, 70.0], [30.0, 40.0])
PIXDIMS = [(1.2, 1.0, 0.9), (1.0, 1.0, 1.0)]
BRAIN_QUANTILE = 0.35   # the skull stage's threshold: this quantile of its own probabilities inside the mask, so that the candidate brain
#                         is a sparse set that falls apart into several pieces on a volume this small


def engine_stage(kw, P, shape_padded, stats, res, **more):
    from bts_amd import infer
    from bts_amd.model import Model
    m = Model(**kw)
    m.build((1,) + tuple(shape_padded) + (2,))
    m.set_weights_from(P)
    return infer.StageSpec(m, torch.tensor(stats[0]), torch.tensor(stats[1]), res, **more)


@pytest.fixture(scope='module')
def two_stage():
    """the 11 x 9 x 14 x 2 two-stage fixture of tests/test_segment_gpu.py, built again here: per pixdim the scan, both stages and
    today's result"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    out = {}
    for pixdim in PIXDIMS:
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
        out[pixdim] = dict(x=x, shape=shape, skull=skull, tumor=tumor, y=y, lab=lab, st=st)
    return out


@pytest.mark.parametrize('pixdim', PIXDIMS)
def test_options_off_change_nothing(two_stage, pixdim):
    from bts_amd import infer
    r = two_stage[pixdim]
    assert r['skull'].largest_component is False
    plain = {'x1mm', 'mask', 'skull_prob', 'x_stripped', 'mask_repadded', 'prob_1mm'}
    assert set(r['st']) == plain and all(isinstance(v, torch.Tensor) for v in r['st'].values())      # the dict callers have always got
    assert r['st'].get('brain_kept') is None and r['st'].get('brain_counts') is None and r['st'].get('postprocess') is None
    y, lab = infer.segment_case(r['tumor'], r['x'], pixdim, skull=r['skull'])
    assert torch.equal(y, r['y']) and torch.equal(lab, r['lab'])
    y, lab, st = infer.segment_case(r['tumor'], r['x'], pixdim, skull=r['skull'], return_stages=True, postprocess=None)
    assert torch.equal(y, r['y']) and torch.equal(lab, r['lab']) and set(st) == plain
    for key in ('skull_prob', 'x_stripped', 'mask_repadded', 'prob_1mm'):
        assert torch.equal(st[key], r['st'][key]), key


@pytest.mark.parametrize('pixdim', PIXDIMS)
def test_skull_stage_keeps_the_largest_component(two_stage, pixdim):
    """'brain_kept' against the restatement applied to the engine's own skull probability and mask, the hand-over against numpy
    x * (1 - p') with p' = 1 at the candidates that were dropped, both bit for bit"""
    from bts_amd import infer
    r = two_stage[pixdim]
    p0, mask = r['st']['skull_prob'].cpu().numpy(), r['st']['mask'].cpu().numpy()
    thr = float(np.quantile(p0[mask > 0], BRAIN_QUANTILE))
    skull = infer.StageSpec(r['skull'].model, r['skull'].mean, r['skull'].std, 4, threshold=thr, largest_component=True)
    y, lab, st = infer.segment_case(r['tumor'], r['x'], pixdim, skull=skull, return_stages=True)
    p = st['skull_prob'].cpu().numpy()
    assert np.array_equal(p.view(np.uint32), p0.view(np.uint32))                      # the stage's own output, as without the option
    cand = ((mask > 0) & (p < np.float32(thr)))[..., 0].astype(np.uint8)
    want, counts = C.remove_components(cand, 2, 2, 26, largest_only=True)
    print('candidate brain: %d voxels in %d components, %d voxels kept' % (int(cand.sum()), counts['components'], int(want.sum())))
    assert counts['components'] >= 2 and counts['removed_voxels'] > 0                 # the fixture gives the step something to do
    kept = st['brain_kept']
    assert kept.dtype == torch.uint8 and tuple(kept.shape) == cand.shape
    assert np.array_equal(kept.cpu().numpy(), want) and st['brain_counts'] == counts
    p2 = np.where(((cand > 0) & (want == 0))[..., None], np.float32(1.0), p).astype(np.float32)
    xo_ref, mo_ref = S.strip(st['x1mm'].cpu().numpy(), p2, mask, r['shape'], S.padded(r['shape'], 8))
    assert np.array_equal(st['x_stripped'].cpu().numpy().view(np.uint32), xo_ref.view(np.uint32))
    assert np.array_equal(st['mask_repadded'].cpu().numpy().view(np.uint32), mo_ref.view(np.uint32))
    assert not torch.equal(st['x_stripped'], r['st']['x_stripped'])
    assert tuple(lab.shape) == VOL and tuple(y.shape) == VOL + (3,)


@pytest.mark.parametrize('pixdim', PIXDIMS)
def test_segment_case_postprocesses_the_labels_on_the_scans_grid(two_stage, pixdim):
    from bts_amd import infer
    r = two_stage[pixdim]
    lab0 = r['lab'].cpu().numpy()
    kw = pick_postprocess(lab0)
    want, counts = C.postprocess_labels(lab0, **kw)
    assert not np.array_equal(want, lab0)
    y, lab, st = infer.segment_case(r['tumor'], r['x'], pixdim, skull=r['skull'], return_stages=True, postprocess=kw)
    assert torch.equal(y, r['y'])                                                     # the probabilities are unchanged
    assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy(), want) and st['postprocess'] == counts
    assert torch.equal(r['lab'], gpu(lab0))                                           # ... and so is the earlier call's map


def pick_postprocess(lab, connectivity=26):
    """the smallest min_component_voxels at which the restatement removes a component of `lab` (2 where the whole tumour is a single
    piece, as the random models of these fixtures give it: the step runs and finds nothing to remove), and an et_min_voxels one above
    the enhancing voxels that are left then: that step has something to do whenever the map holds label 4"""
    comp = C.components3d(lab, 14, 4, connectivity)
    size = C.sizes(comp)[0]
    m = int(size[size > 0].min()) + 1 if int((size > 0).sum()) >= 2 else 2
    after = C.postprocess_labels(lab, min_component_voxels=m, connectivity=connectivity)[0]
    n_et = int((after >= 3).sum())
    return {'min_component_voxels': m, 'et_min_voxels': n_et + 1 if n_et else 0, 'connectivity': connectivity}


# ---- the command -------------------------------------------------------------------------------------------------------------------
def write_case(folder, vol, seed, affine):
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


def test_command_with_and_without_the_flags(tmp_path, capsys):
    """three labelled cases (one with non-unit pixdim), two checkpoints.  Without the flags: what segment_case and label_scores give by
    hand, byte for byte.  With them: the restatement applied to the first run's masks, the scores recomputed from it, and --workers 0
    against --workers 2."""
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti
    from bts_amd import test as T
    data = tmp_path / 'data'
    affines = {'a': np.eye(4), 'b': np.diag([1.2, 1.0, 0.9, 1.0]), 'c': np.eye(4)}
    truth = {name: write_case(str(data / name), VOL, 5 + i, affines[name]) for i, name in enumerate('abc')}
    write_model(str(tmp_path / 'tumor'), TUMOR_KW, (32, 16, 16), True, SEED + 20)
    write_model(str(tmp_path / 'skull'), SKULL_KW, S.padded(VOL, 4), False, SEED + 10)
    for name, (mean, std) in (('tp.npy', TUMOR_STATS), ('sp.npy', SKULL_STATS)):
        np.save(str(tmp_path / name), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                       'norm': {'mean': np.array(mean).reshape(1, 1, 1, 2), 'std': np.array(std).reshape(1, 1, 1, 2)}})
    base = ['--in_locs', str(data), '--modalities', 't1ce,flair', '--truth', 'seg', '--gpu',
            '--tumor_model', str(tmp_path / 'tumor'), '--tumor_prepro', str(tmp_path / 'tp.npy'),
            '--skull_model', str(tmp_path / 'skull'), '--skull_prepro', str(tmp_path / 'sp.npy')]

    # without the flags: the existing behaviour, done by hand
    plain = tmp_path / 'plain'
    res = T.run(T.parse_args(base + ['--workers', '0', '--out_loc', str(plain)]))
    assert res['postprocess'] == [] and res['cases'] == 3 and res['scored'] == 3
    assert 'Post-processing' not in capsys.readouterr().out
    args = T.parse_args(base)
    tumor = skull = None
    masks, rows, conf = {}, [], np.zeros((4, 4), dtype=np.int64)
    for name, path in T.find_cases(args.in_locs):
        case = T.decode_case(path, args.modalities, args.truth)
        x, y = T.upload_case(case, dev())
        pixdim = tuple(float(v) for v in case['pixdim'][1:4])
        if tumor is None:
            tumor = T.load_stage(args.tumor_model, args.tumor_prepro, args, tuple(x.shape[:3]))
            skull = T.load_stage(args.skull_model, args.skull_prepro, args, tuple(x.shape[:3]))
        _, lab = infer.segment_case(tumor, x, pixdim, skull=skull, order=args.order)
        hand = tmp_path / ('hand_%s.nii' % name)
        nifti.save(str(hand), lab.cpu().numpy(), case['affine'])
        assert read(str(hand)) == read(str(plain / name / 'mask.nii')), name
        masks[name] = lab.cpu().numpy()
        s = infer.label_scores(y, lab, 4)
        assert np.array_equal(y.cpu().numpy(), truth[name])
        rows.append(T.score_row(name, s))
        conf += s['confusion']
    head = ['case', 'macro', 'micro', 'dice_1', 'dice_2', 'dice_3', 'wt', 'tc', 'et']
    rows = [head] + rows + [T.score_row('total', infer.scores_from_confusion(conf))]
    assert read(str(plain / 'scores.csv'), 'r') == ''.join(','.join(r) + '\n' for r in rows)

    # with the flags, chosen so that the restatement changes the first case that holds label 4 (and whatever else it changes)
    first = next(name for name in 'abc' if (masks[name] == 4).any())
    kw = pick_postprocess(masks[first], 18)
    want = {name: C.postprocess_labels(m, **kw) for name, m in masks.items()}
    assert not np.array_equal(want[first][0], masks[first])
    flags = ['--min_component_voxels', str(kw['min_component_voxels']), '--et_min_voxels', str(kw['et_min_voxels']),
             '--component_connectivity', '18']
    outs = []
    for workers in (0, 2):
        out = tmp_path / ('flag%d' % workers)
        res = T.run(T.parse_args(base + flags + ['--workers', str(workers), '--out_loc', str(out)]))
        assert res['postprocess'] == [(name, want[name][1]) for name in 'abc']
        outs.append(out)
    assert capsys.readouterr().out.count('. Post-processing: ') == 6
    conf[:] = 0
    rows = [head]
    for name in 'abc':
        assert read(str(outs[0] / name / 'mask.nii')) == read(str(outs[1] / name / 'mask.nii')), name
        lab, _ = nifti.load(str(outs[0] / name / 'mask.nii'))
        assert lab.dtype == np.uint8 and np.array_equal(lab, want[name][0]), name
        s = infer.label_scores(truth[name], want[name][0])
        rows.append(T.score_row(name, s))
        conf += s['confusion']
    rows.append(T.score_row('total', infer.scores_from_confusion(conf)))
    text = read(str(outs[0] / 'scores.csv'), 'r')
    assert text == read(str(outs[1] / 'scores.csv'), 'r') == ''.join(','.join(r) + '\n' for r in rows)
    assert text != read(str(plain / 'scores.csv'), 'r')

    # the skull stage's option alone: its counts per case, and the masks of segment_case with the option set by hand
    out = tmp_path / 'brain'
    res = T.run(T.parse_args(base + ['--skull_largest_component', '--workers', '0', '--out_loc', str(out)]))
    assert [n for n, _ in res['postprocess']] == ['a', 'b', 'c']
    skull.largest_component = True
    for (name, path), (_, counts) in zip(T.find_cases(args.in_locs), res['postprocess']):
        case = T.decode_case(path, args.modalities, args.truth)
        x, _ = T.upload_case(case, dev())
        _, lab, st = infer.segment_case(tumor, x, tuple(float(v) for v in case['pixdim'][1:4]), skull=skull, return_stages=True)
        assert counts == {'brain_' + k: v for k, v in st['brain_counts'].items()} and counts['brain_components'] >= 1
        assert np.array_equal(nifti.load(str(out / name / 'mask.nii'))[0], lab.cpu().numpy()), name
