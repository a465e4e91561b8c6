"""-m gpu: csrc/surface.hip (bts_region_surface, bts_edt3d_sq, bts_masked_select) bit for bit against the NumPy restatement of
tests/surface_ref.py, infer.surface_scores against known answers and against that restatement, and `python -m bts_amd.test
--surface_metrics` end to end on three tiny cases.

Shapes: a line shorter than a wave (5,6,7), lines of 65 and 70 (a wave and a tail), a line of 300 (longer than a 256-thread
workgroup) and an extent of 1."""
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
import segment_ref as S  # noqa: E402
import surface_ref as H  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

SHAPES = [(5, 6, 7), (1, 9, 70), (17, 3, 300), (33, 70, 65)]
SPACINGS = [(1.0, 1.0, 1.0), H.widened((1.2, 1.0, 0.9))]
SPACING = SPACINGS[1]
SENTINEL = -777.0


def dev():
    return torch.device('cuda', 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- bts_edt3d_sq ---------------------------------------------------------------------------------------------------------------
def feature_sets(shape):
    rnd = (np.random.default_rng(11).random(shape) < 0.01).astype(np.uint8)
    rnd[-1, -1, -1] = 1
    corner = np.zeros(shape, np.uint8)
    corner[0, 0, 0] = 1
    return {'random': rnd, 'corner': corner, 'none': np.zeros(shape, np.uint8)}


@pytest.mark.parametrize('spacing', SPACINGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_edt3d_sq_is_bit_equal_to_the_restatement(shape, spacing):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    for name, f in feature_sets(shape).items():
        ref = H.edt_sq(f, spacing)
        out = torch.full(shape, SENTINEL, dtype=torch.float64, device=dev())
        got = ops.edt3d_sq(gpu(f), spacing, out=out)
        assert got is out
        assert np.array_equal(bits(got.cpu().numpy()), bits(ref)), name
        if name == 'none':
            assert np.all(np.isinf(ref)) and np.all(ref > 0)
    assert np.array_equal(bits(ops.edt3d_sq(gpu(f), spacing).cpu().numpy()), bits(ref))       # without out=


def test_edt3d_sq_refuses_bad_arguments():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    f = torch.zeros((4, 5, 6), dtype=torch.uint8, device=dev())
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.edt3d_sq(f, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match='float64'):
        ops.edt3d_sq(f, out=torch.zeros((4, 5, 6), device=dev()))
    with pytest.raises(ValueError, match='uint8'):
        ops.edt3d_sq(f.float())
    with pytest.raises(ValueError, match='uint8'):
        ops.edt3d_sq(f.cpu())


# ---- bts_region_surface ---------------------------------------------------------------------------------------------------------
def label_volume(shape, seed):
    """piecewise-constant blobs of labels 0, 1, 2, 3, 4 and 255 plus single-voxel noise"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    lab = np.zeros(shape, np.uint8)
    for value in (1, 2, 4, 3, 255, 1):
        c = [rng.integers(0, n) for n in shape]
        r = [max(1.5, 0.35 * n) for n in shape]
        lab[sum(((gi - ci) / ri) ** 2 for gi, ci, ri in zip(g, c, r)) < 1.0] = value
    noise = rng.random(shape) < 0.02
    lab[noise] = np.array([0, 1, 2, 3, 4, 255], np.uint8)[rng.integers(0, 6, size=int(noise.sum()))]
    return lab


@pytest.mark.parametrize('k', [4, 8])
@pytest.mark.parametrize('shape', SHAPES)
def test_region_surface_equals_the_helper(shape, k):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    lab = label_volume(shape, 3)
    assert {3, 4, 255} <= set(np.unique(lab).tolist())
    lg = gpu(lab)
    regions = list(H.BRATS.values()) + [1 << c for c in range(k)] + [(1 << k) - 1, 0]
    for cm in regions:
        ref = H.surface(H.region(lab, k, cm))
        out = torch.full(shape, 77, dtype=torch.uint8, device=dev())
        surf, count = ops.region_surface(lg, k, cm, out=out)
        assert surf is out and np.array_equal(surf.cpu().numpy(), ref.astype(np.uint8)), cm
        assert int(count.item()) == int(ref.sum())
        ops.region_surface(lg, k, cm, out=out, count=count)                         # a second call into the same count: the sum
        assert int(count.item()) == 2 * int(ref.sum())
    full = np.full(shape, 2, np.uint8)                                                  # a full volume: its shell
    surf, count = ops.region_surface(gpu(full), k, 0b0100)
    shell = np.ones(shape, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(surf.cpu().numpy(), shell.astype(np.uint8)) and int(count.item()) == int(shell.sum())
    surf, count = ops.region_surface(gpu(np.zeros(shape, np.uint8)), k, 0b1110)         # an empty one
    assert not surf.any().item() and int(count.item()) == 0


def test_region_surface_off_a_4_byte_boundary_and_bad_arguments():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    shape = (5, 6, 7)
    lab = label_volume(shape, 4)
    ref = H.surface(H.region(lab, 4, 0b1110)).astype(np.uint8)
    buf = torch.zeros(lab.size + 8, dtype=torch.uint8, device=dev())
    obuf = torch.full((lab.size + 8,), 77, dtype=torch.uint8, device=dev())
    for off_l, off_o in ((1, 0), (0, 3), (2, 2)):
        lv = buf[off_l:off_l + lab.size].view(shape)
        lv.copy_(gpu(lab))
        obuf.fill_(77)
        surf, count = ops.region_surface(lv, 4, 0b1110, out=obuf[off_o:off_o + lab.size].view(shape))
        assert np.array_equal(surf.cpu().numpy(), ref) and int(count.item()) == int(ref.sum())
        rest = obuf.cpu().numpy()
        assert np.all(rest[:off_o] == 77) and np.all(rest[off_o + lab.size:] == 77)     # nothing outside the volume is written
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.region_surface(gpu(lab), 9, 1)
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.region_surface(gpu(lab), 4, 16)
    with pytest.raises(ValueError, match=r'\(D,H,W\)'):
        ops.region_surface(gpu(lab.reshape(-1)))


# ---- bts_masked_select ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('density', [0.01, 1.0])
@pytest.mark.parametrize('n', [1, 2, 15, 4097, 2 ** 20 + 3])
def test_masked_select_is_bit_equal_to_sort(n, density):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(n)
    steps = np.array([0.0, 0.0, 0.0] + [float(np.float64(s) * i) for s in SPACING for i in range(1, 6)])
    v = np.square(steps[rng.integers(0, len(steps), size=n)]) + np.square(steps[rng.integers(0, len(steps), size=n)])
    v[rng.random(n) < 0.001] = np.inf
    mask = (rng.random(n) < density).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
    if density == 1.0:
        assert mask.all()
    sel = np.sort(v[mask != 0])
    m = len(sel)
    ranks = [0, m // 2, max(m - 1, 0), m]
    ref = np.array([sel[r] if r < m else np.nan for r in ranks])
    vg, mg = gpu(v), gpu(mask)
    got1 = ops.masked_select(vg, mg, ranks).cpu().numpy()
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device=dev())
    got2 = ops.masked_select(vg, mg, ranks, out=out)
    assert got2 is out
    got2 = got2.cpu().numpy()
    assert np.array_equal(np.isnan(got1), np.isnan(ref)) and math.isnan(got1[3])
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(got1)[ok], bits(ref)[ok]), (got1, ref)
    assert bits(got1).tobytes() == bits(got2).tobytes()                                 # two runs: the same bytes
    none = ops.masked_select(vg, torch.zeros_like(mg), [0, 1]).cpu().numpy()            # an all-zero mask
    assert np.all(np.isnan(none))
    if n > 8:                                                                            # eight ranks at once, off a 4-byte boundary
        ranks8 = [int(r) for r in np.linspace(0, max(m - 1, 0), 8)]
        sel1 = np.sort(v[1:][mask[1:] != 0])
        got8 = ops.masked_select(vg[1:], mg[1:], ranks8).cpu().numpy()
        ref8 = np.array([sel1[r] if r < len(sel1) else np.nan for r in ranks8])
        ok = ~np.isnan(ref8)
        assert np.array_equal(np.isnan(got8), ~ok) and np.array_equal(bits(got8)[ok], bits(ref8)[ok])


def test_masked_select_refuses_bad_arguments():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    v = torch.zeros(10, dtype=torch.float64, device=dev())
    m = torch.ones(10, dtype=torch.uint8, device=dev())
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.masked_select(v, m, [0, -1])
    with pytest.raises(RuntimeError):
        ops.masked_select(v, m, list(range(9)))
    with pytest.raises(ValueError, match='10 values and 9 mask bytes'):
        ops.masked_select(v, m[:9], [0])
    with pytest.raises(ValueError, match='float64'):
        ops.masked_select(v.float(), m, [0])
    assert np.all(np.isnan(ops.masked_select(v[:0], m[:0], [0, 3]).cpu().numpy()))      # no values at all


# ---- infer.surface_scores -------------------------------------------------------------------------------------------------------
def test_surface_scores_known_answers():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    t = np.zeros((8, 8, 12), np.uint8)
    p = np.zeros((8, 8, 12), np.uint8)
    t[2, 3, 4] = 1
    p[5, 3, 8] = 1
    want = math.sqrt((3 * SPACING[0]) ** 2 + (4 * SPACING[2]) ** 2)
    for a, b in ((t, p), (gpu(t), gpu(p))):                                              # numpy and device tensors alike
        s = infer.surface_scores(a, b, SPACING)
        assert s['hd95'][0] == pytest.approx(want, rel=1e-12) and s['hd'][0] == pytest.approx(want, rel=1e-12)
        assert s['hd95_directed'][0] == pytest.approx((want, want), rel=1e-12) and s['surface_voxels'][0] == (1, 1)
        assert s['hd95_wt'] == pytest.approx(want, rel=1e-12) and s['hd_tc'] == pytest.approx(want, rel=1e-12)
        assert math.isnan(s['hd95'][1]) and math.isnan(s['hd95_et']) and math.isnan(s['hd_et'])      # empty in both maps
        assert set(s) == {'hd95', 'hd', 'hd95_directed', 'surface_voxels', 'hd95_wt', 'hd95_tc', 'hd95_et', 'hd_wt', 'hd_tc', 'hd_et'}
    same = infer.surface_scores(t, t, SPACING)
    assert same['hd95'][0] == 0.0 and same['hd'][0] == 0.0 and same['hd95_wt'] == 0.0
    one = infer.surface_scores(t, np.zeros_like(t), SPACING)
    assert one['hd95'][0] == math.inf and one['hd'][0] == math.inf and one['hd95_wt'] == math.inf and one['surface_voxels'][0] == (1, 0)
    assert math.isnan(one['hd95'][2])
    cube = np.zeros((10, 10, 12), np.uint8)
    cube[2:8, 2:8, 2:8] = 4
    moved = np.roll(cube, 2, axis=2)
    s = infer.surface_scores(cube, moved, SPACING)
    assert s['hd'][2] == pytest.approx(2 * SPACING[2], rel=1e-12) and s['hd_et'] == s['hd'][2] and s['hd95_et'] == s['hd95'][2]
    assert 0.0 < s['hd95'][2] <= s['hd'][2]
    s2 = infer.surface_scores(cube, moved, SPACING, n_classes=2)                         # K = 2: one foreground class, no regions
    assert set(s2) == {'hd95', 'hd', 'hd95_directed', 'surface_voxels'} and s2['hd'] == [s['hd'][2]]
    with pytest.raises(ValueError, match=r'\(8, 8, 12\).*\(10, 10, 12\)'):
        infer.surface_scores(t, cube, SPACING)


def blobs(shape, shift, seed):
    """nested blobs with labels 2 (outer), 1 and 4 (inner); `shift` moves them, and a few voxels are perturbed"""
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    c = [n / 2.0 + s for n, s in zip(shape, shift)]
    r2 = sum(((gi - ci) / (0.4 * n)) ** 2 for gi, ci, n in zip(g, c, shape))
    lab = np.zeros(shape, np.uint8)
    lab[r2 < 1.0] = 2
    lab[r2 < 0.45] = 1
    lab[r2 < 0.12] = 4
    rng = np.random.default_rng(seed)
    flip = rng.random(shape) < 0.01
    lab[flip] = np.array([0, 1, 2, 4], np.uint8)[rng.integers(0, 4, size=int(flip.sum()))]
    return lab


def test_surface_scores_equal_the_helper():
    import bts_amd  # noqa: F401
    from bts_amd import infer, ops
    shape = (24, 20, 18)
    t, p = blobs(shape, (0, 0, 0), 1), blobs(shape, (1.5, -1.0, 2.0), 2)
    got = infer.surface_scores(t, p, SPACING)
    regions = [('class', c, 1 << c) for c in (1, 2, 3)] + [('region', name, cm) for name, cm in H.BRATS.items()]
    for kind, key, cm in regions:
        tm, pm = H.region(t, 4, cm), H.region(p, 4, cm)
        ref = H.hd95(tm, pm, SPACING)
        # every order statistic the score uses, bit for bit: the device's transforms and selection on this region
        d_pt, d_tp = H.directed_sq(tm, pm, SPACING)
        st, sp = gpu(H.surface(tm).astype(np.uint8)), gpu(H.surface(pm).astype(np.uint8))
        dist = torch.cat([ops.edt3d_sq(st, SPACING).reshape(-1), ops.edt3d_sq(sp, SPACING).reshape(-1)])
        mask = torch.cat([sp.reshape(-1), st.reshape(-1)])
        n = t.size
        for values, vg, mg in ((np.concatenate([d_pt, d_tp]), dist, mask), (d_pt, dist[:n], mask[:n]), (d_tp, dist[n:], mask[n:])):
            m = len(values)
            pos = 0.95 * (m - 1)
            ranks = [int(np.floor(pos)), int(np.ceil(pos)), m - 1]
            assert np.array_equal(bits(ops.masked_select(vg, mg, ranks).cpu().numpy()), bits(np.sort(values)[ranks])), (key, m)
        if kind == 'class':
            mine = (got['hd95'][key - 1], got['hd'][key - 1], got['hd95_directed'][key - 1], got['surface_voxels'][key - 1])
        else:
            mine = (got['hd95_' + key], got['hd_' + key], None, None)
        assert ref['hd'] > 0.0 and mine[0] == pytest.approx(ref['hd95'], rel=1e-12) and mine[1] == pytest.approx(ref['hd'], rel=1e-12)
        if kind == 'class':
            assert mine[2] == pytest.approx(ref['hd95_directed'], rel=1e-12) and mine[3] == ref['surface_voxels']


# ---- the command -----------------------------------------------------------------------------------------------------------------
TUMOR_KW = dict(base_filters=8, groups=2, reduction=2, depth=3)
VOL, SEED = (11, 9, 14), 5
TUMOR_STATS = ([60.0, 70.0], [30.0, 40.0])
HEAD = ['case', 'macro', 'micro', 'dice_1', 'dice_2', 'dice_3', 'wt', 'tc', 'et']
EXTRA = ['hd95_wt', 'hd95_tc', 'hd95_et', 'sens_wt', 'sens_tc', 'sens_et', 'spec_wt', 'spec_tc', 'spec_et']


def write_case(folder, vol, seed, affine, seg):
    from bts_amd import nifti
    os.makedirs(folder)
    x = S.scan_like(vol, seed)
    nifti.save(os.path.join(folder, 'c_t1ce.nii.gz'), x[..., 0], affine)
    nifti.save(os.path.join(folder, 'c_flair.nii'), x[..., 1], affine)
    y = None
    if seg is not None:
        y = seg
        nifti.save(os.path.join(folder, 'c_seg.nii.gz'), y.astype(np.int16), affine)
    return y


def write_model(folder, kw, build, seed):
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    cfg = R.default_config(**kw)
    m = Model(**kw)
    m.build((1,) + tuple(build) + (2,))
    m.set_weights_from(S.randomised_params(cfg, tuple(build), seed))
    save_checkpoint(folder, m)
    save_train_args(folder, {'model_args': dict(kw), 'crop_size': list(build)})


def test_command_with_surface_metrics(tmp_path, capsys):
    """three labelled cases (one with non-unit pixdim, one whose truth has no enhancing tumour: an infinite or undefined ET distance),
    with the flag at --workers 0 and 2, and without it"""
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti
    from bts_amd import test as T
    data = tmp_path / 'data'
    seg_a = blobs(VOL, (0, 0, 0), 1)
    seg_b = blobs(VOL, (1.0, 0.0, -1.0), 2)
    seg_c = np.where(blobs(VOL, (0, 1.0, 0), 3) == 4, 1, blobs(VOL, (0, 1.0, 0), 3)).astype(np.uint8)
    affines = {'a': np.eye(4), 'b': np.diag([1.2, 1.0, 0.9, 1.0]), 'c': np.eye(4)}
    truth = {'a': write_case(str(data / 'a'), VOL, 5, affines['a'], seg_a),
             'b': write_case(str(data / 'b'), VOL, 6, affines['b'], seg_b),
             'c': write_case(str(data / 'c'), VOL, 7, affines['c'], seg_c)}
    write_model(str(tmp_path / 'tumor'), TUMOR_KW, (32, 16, 16), SEED + 20)
    np.save(str(tmp_path / 'tp.npy'), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                       'norm': {'mean': np.array(TUMOR_STATS[0]).reshape(1, 1, 1, 2),
                                                'std': np.array(TUMOR_STATS[1]).reshape(1, 1, 1, 2)}})
    base = ['--in_locs', str(data), '--modalities', 't1ce,flair', '--truth', 'seg', '--gpu', '--tumor_model', str(tmp_path / 'tumor'),
            '--tumor_prepro', str(tmp_path / 'tp.npy')]
    outs = {}
    for tag, more in (('w0', ['--surface_metrics', '--workers', '0']), ('w2', ['--surface_metrics', '--workers', '2']),
                      ('plain', ['--workers', '0'])):
        outs[tag] = tmp_path / tag
        assert T.main(base + more + ['--out_loc', str(outs[tag])]) == 0
    text = capsys.readouterr().out
    assert text.count('3 cases segmented (3 scored)') == 3 and text.count('a. Macro: ') == 3
    assert text.count('a. HD95 WT: ') == 2 and text.count('region distances infinite') == 2
    csv = {tag: open(str(o / 'scores.csv')).read() for tag, o in outs.items()}
    assert csv['w0'] == csv['w2']                                                        # byte-equal across worker counts
    rows = [r.split(',') for r in csv['w0'].strip().split('\n')]
    assert rows[0] == HEAD + EXTRA and [r[0] for r in rows] == ['case', 'a', 'b', 'c', 'total'] and all(len(r) == 18 for r in rows)
    # without the flag: the pinned header, and the same file with the new columns cut off
    plain = [r.split(',') for r in csv['plain'].strip().split('\n')]
    assert plain[0] == HEAD and plain == [r[:9] for r in rows]
    assert csv['plain'] == ''.join(','.join(r[:9]) + '\n' for r in rows)
    conf = np.zeros((4, 4), dtype=np.int64)
    hd, n_inf = {k: [] for k in EXTRA[:3]}, 0
    for row, case in zip(rows[1:4], ('a', 'b', 'c')):
        lab, hdr = nifti.load(str(outs['w0'] / case / 'mask.nii'))
        assert open(str(outs['w0'] / case / 'mask.nii'), 'rb').read() == open(str(outs['plain'] / case / 'mask.nii'), 'rb').read()
        s = infer.label_scores(truth[case], lab)
        pixdim = tuple(float(v) for v in T.decode_case(str(data / case), ['t1ce', 'flair'], '')['pixdim'][1:4])   # as run() takes it
        assert pixdim == pytest.approx((1.2, 1.0, 0.9) if case == 'b' else (1.0, 1.0, 1.0), rel=1e-6)
        d = infer.surface_scores(truth[case], lab, pixdim)
        rates = infer.region_rates_from_confusion(s['confusion'])
        assert row[:9] == T.score_row(case, s)
        assert row[9:12] == ['%.6f' % d[k] for k in EXTRA[:3]] and row[12:] == ['%.6f' % rates[k] for k in EXTRA[3:]]
        for k in EXTRA[:3]:
            hd[k].append(d[k])
            n_inf += int(math.isinf(d[k]))
        conf += s['confusion']
    assert '; %d region distances infinite' % n_inf in text
    total = infer.region_rates_from_confusion(conf)
    assert rows[4][:9] == T.score_row('total', infer.scores_from_confusion(conf))
    for i, k in enumerate(EXTRA[:3]):
        finite = [v for v in hd[k] if math.isfinite(v)]
        assert rows[4][9 + i] == '%.6f' % (float(np.mean(finite)) if finite else float('nan'))
    assert rows[4][12:] == ['%.6f' % total[k] for k in EXTRA[3:]]
    assert any(math.isfinite(v) and v > 0.0 for k in EXTRA[:3] for v in hd[k])          # the distances are not all degenerate
