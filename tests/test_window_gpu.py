"""-m gpu: csrc/window.hip (bts_window_gather, bts_window_accumulate, bts_window_occupancy) against the float64 restatement of
tests/window_ref.py, the windowed TestTimeAugmentor end to end against the fp64 oracle run per window and flip, and
`python -m bts_amd.test --window` on a tiny case."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import window_ref as WR  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

ULP = 2.0 ** -23                    # of 1.0 in float32

# (volume, roi): a window inside, a window hanging over every axis, an odd row length, and rows long enough for several workgroups
SHAPES = [((5, 6, 7), (4, 4, 4)), ((5, 6, 7), (8, 8, 8)), ((3, 9, 33), (2, 4, 16)), ((3, 25, 70), (2, 24, 64))]


def dev():
    return torch.device('cuda', 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def some_starts(rng, vol, roi, n):
    """n window starts of the plan's kind: inside the volume, the last ones reaching (or hanging over) its end"""
    starts = WR.plan(vol, roi)[0]
    return [tuple(int(starts[a][rng.integers(0, len(starts[a]))]) for a in range(3)) for _ in range(n)]


# ---- gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 2, 3, 4])
@pytest.mark.parametrize('vol,roi', SHAPES)
def test_gather_matches_the_reference(vol, roi, c):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(11 + c)
    x = (rng.standard_normal(vol + (c,)) * 40.0 + 100.0).astype(np.float32)
    xg = torch.from_numpy(x).to(dev())
    # one job, no flip, no normalisation: the bits of the slice, zero beyond the volume's end
    for start in set(some_starts(rng, vol, roi, 4)) | {(0, 0, 0), (vol[0] - 1, vol[1] - 1, vol[2] - 1)}:
        out = torch.full((1,) + roi + (c,), float('nan'), device=dev())
        ops.window_gather(xg, roi, [start], [0], [[0.0] * c], [[1.0] * c], out=out)
        ref = WR.gather_ref(x, roi, start, 0, [0.0] * c, [1.0] * c).astype(np.float32)
        assert np.array_equal(out[0].cpu().numpy(), ref), start
    for flip in range(8):
        for b in (1, 3):
            starts = some_starts(rng, vol, roi, b)
            flips = [flip] + [int(f) for f in rng.integers(0, 8, size=b - 1)]
            means = (rng.standard_normal((b, c)) * 20.0 + 90.0).astype(np.float32)
            stds = (rng.random((b, c)) * 30.0 + 20.0).astype(np.float32)
            out = torch.full((b,) + roi + (c,), float('nan'), device=dev())
            got = ops.window_gather(xg, roi, starts, flips, means.tolist(), stds.tolist(), out=out)
            assert got is out
            got = got.cpu().numpy()
            assert not np.isnan(got).any(), 'an element of the output was not written'
            for j in range(b):
                ref = WR.gather_ref(x, roi, starts[j], flips[j], means[j], stds[j])
                assert np.allclose(got[j], ref, rtol=1e-6, atol=1e-6), (flip, b, j, float(np.abs(got[j] - ref).max()))
    assert np.array_equal(ops.window_gather(xg, roi, [(0, 0, 0)], [5], [[1.0] * c], [[2.0] * c]).cpu().numpy()[0],
                          WR.gather_ref(x, roi, (0, 0, 0), 5, [1.0] * c, [2.0] * c).astype(np.float32))      # exact in fp32: /2


def test_ops_refuse_bad_tensors():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x = torch.zeros((4, 4, 4, 2), device=dev())
    with pytest.raises(ValueError):
        ops.window_gather(x[:, :, ::2], (2, 2, 2), [(0, 0, 0)], [0], [[0.0, 0.0]], [[1.0, 1.0]])
    with pytest.raises(ValueError):
        ops.window_gather(x, (2, 2, 2), [(0, 0, 0)], [0], [[0.0]], [[1.0]])
    with pytest.raises(ValueError):
        ops.window_gather(x, (2, 2, 2), [(0, 0, 0)], [0], [[0.0, 0.0]], [[1.0, 1.0]], out=torch.zeros((1, 2, 2, 2, 3), device=dev()))
    with pytest.raises(RuntimeError):
        ops.window_gather(x, (2, 2, 2), [(4, 0, 0)], [0], [[0.0, 0.0]], [[1.0, 1.0]])       # a start outside the volume
    t = [torch.ones((1, 2), device=dev())] * 3
    with pytest.raises(ValueError):
        ops.window_accumulate(torch.zeros((1, 2, 2, 2, 3), device=dev()), x, t, [(0, 0, 0)], [0], [(0, 0, 0)])      # K differs
    with pytest.raises(RuntimeError):
        ops.window_accumulate(x.view(1, 4, 4, 4, 2), x, [torch.ones((1, 4), device=dev())] * 3, [(0, 0, 0)], [0], [(0, 0, 0)])   # aliasing
    with pytest.raises(ValueError):
        ops.window_occupancy(x, (2, 2, 2), ([0], [0], [0]))


# ---- accumulate ------------------------------------------------------------------------------------------------------------------
def accumulate_case(vol, roi, k, seed, njobs=5):
    """5 jobs drawn from the plan's windows (they overlap; the last windows reach the volume's end or hang over it)"""
    rng = np.random.default_rng(seed)
    starts, tables = WR.plan(vol, roi)
    tables = [t.astype(np.float32) for t in tables]
    rows = [tuple(int(rng.integers(0, len(starts[a]))) for a in range(3)) for _ in range(njobs)]
    rows[-1] = tuple(len(starts[a]) - 1 for a in range(3))                       # the far corner: at or over the end on every axis
    rows[1] = rows[0]                                                            # the same window twice
    at = [tuple(starts[a][r[a]] for a in range(3)) for r in rows]
    flips = [int(f) for f in rng.integers(0, 8, size=njobs)]
    pred = (rng.random((njobs,) + roi + (k,)) * 0.9 + 0.05).astype(np.float32)
    acc0 = (1.0 + 1e-3 * np.arange(int(np.prod(vol)) * k, dtype=np.float64).reshape(vol + (k,)) % 0.37).astype(np.float32)
    return tables, rows, at, flips, pred, acc0


@pytest.mark.parametrize('k', [1, 3, 4])
@pytest.mark.parametrize('vol,roi', SHAPES)
def test_accumulate_matches_the_reference_and_does_not_depend_on_the_batching(vol, roi, k):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    tables, rows, at, flips, pred, acc0 = accumulate_case(vol, roi, k, 23 + k)
    tg = [torch.from_numpy(t).to(dev()) for t in tables]
    pg = torch.from_numpy(pred).to(dev())
    scale = float(np.float32(1.0 / 3.0))
    ref = acc0.astype(np.float64)
    touched = np.zeros(vol, dtype=bool)
    for j in range(len(rows)):
        WR.accumulate_ref(ref, pred[j], tables, at[j], flips[j], rows[j], scale)
        touched[at[j][0]:at[j][0] + roi[0], at[j][1]:at[j][1] + roi[1], at[j][2]:at[j][2] + roi[2]] = True
    one = torch.from_numpy(acc0).to(dev())
    assert ops.window_accumulate(pg, one, tg, at, flips, rows, scale=scale) is one
    got = one.cpu().numpy()
    # voxels outside every window of the launch (the outside of the bounding box among them) keep their bits
    assert np.array_equal(got.view(np.int32)[~touched], acc0.view(np.int32)[~touched])
    # all terms are positive: at most 4 roundings per product and one per addition, (4 + 5) 2^-24 < 1e-6 relative
    err = np.abs(got.astype(np.float64) - ref) / np.abs(ref)
    assert float(err.max()) <= 1e-6, 'max relative error %.3e' % float(err.max())
    assert touched.any() and float(np.abs(got - acc0)[touched].max()) > 0.0
    # one launch of 5 jobs == 5 launches of one job, bit for bit
    step = torch.from_numpy(acc0).to(dev())
    for j in range(len(rows)):
        ops.window_accumulate(pg[j:j + 1], step, tg, at[j:j + 1], flips[j:j + 1], rows[j:j + 1], scale=scale)
    assert torch.equal(bits(step), bits(one))
    # ... and == 2 + 3
    split = torch.from_numpy(acc0).to(dev())
    ops.window_accumulate(pg[:2], split, tg, at[:2], flips[:2], rows[:2], scale=scale)
    ops.window_accumulate(pg[2:], split, tg, at[2:], flips[2:], rows[2:], scale=scale)
    assert torch.equal(bits(split), bits(one))


@pytest.mark.parametrize('mode', ['gaussian', 'constant'])
@pytest.mark.parametrize('vol,roi,k', [((5, 6, 7), (4, 4, 4), 3), ((5, 6, 7), (8, 8, 8), 1), ((13, 9, 33), (8, 4, 16), 4), ((3, 25, 70), (2, 24, 64), 3)])
def test_a_full_plan_of_ones_sums_to_one(vol, roi, k, mode):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    starts, tables = WR.plan(vol, roi, 0.5, mode)
    tg = [torch.from_numpy(t.astype(np.float32)).to(dev()) for t in tables]
    wins = [(iz, iy, ix) for iz in range(len(starts[0])) for iy in range(len(starts[1])) for ix in range(len(starts[2]))]
    acc = torch.zeros(vol + (k,), device=dev())
    cap = ops.window_batch_max()
    for j0 in range(0, len(wins), cap):
        rows = wins[j0:j0 + cap]
        ones = torch.ones((len(rows),) + roi + (k,), device=dev())
        ops.window_accumulate(ones, acc, tg, [tuple(starts[a][r[a]] for a in range(3)) for r in rows], [0] * len(rows), rows, scale=1.0)
    # windows per voxel from the plan: per term three rounded table entries and two rounded products (2.5 ulp), half an ulp per addition
    cover = [WR.axis_coverage(vol[a], starts[a], roi[a]) for a in range(3)]
    nwin = cover[0][:, None, None] * cover[1][None, :, None] * cover[2][None, None, :]
    assert int(nwin.min()) >= 1 and int(nwin.max()) > 1 or len(wins) == 1
    err = np.abs(acc.cpu().numpy().astype(np.float64) - 1.0)
    assert np.all(err <= 4.0 * ULP * nwin[..., None]), 'max |sum - 1| = %.3e at %d windows' % (float(err.max()), int(nwin.max()))


# ---- occupancy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vol,roi', SHAPES + [((13, 9, 33), (8, 4, 16))])
def test_occupancy_is_exact(vol, roi):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(5)
    mask = (rng.random(vol + (1,)) > 0.6).astype(np.float32)
    mask[..., :min(roi[2], vol[2] - 1), :] = 0.0                                 # an empty slab one window wide
    mask[0, 0, vol[2] - 1, 0] = 1.0
    mask[vol[0] - 1, vol[1] - 1, vol[2] - 1, 0] = -1.0                            # not > 0
    starts = WR.plan(vol, roi)[0]
    ref = WR.occupancy_ref(mask, roi, starts)
    out = torch.full(ref.shape, -7, dtype=torch.int32, device=dev())
    got = ops.window_occupancy(torch.from_numpy(mask).to(dev()), roi, starts, out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), ref)
    assert (ref == 0).any() or len(starts[2]) == 1
    assert int(ref.max()) > 0


# ---- end to end against the fp64 oracle ------------------------------------------------------------------------------------------
def randomised_params(cfg, crop, seed):
    """oracle ParamSet with every gamma/beta/bias randomised (gamma_2 = 0 at init would hide the conv branch: F6)"""
    P = R.build_params(cfg, crop, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in P:
        if k.endswith('_b'):
            P[k] = torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.1
        if k.endswith('_g'):
            P[k] = 1.0 + torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.3
    for k in P:  # fp32-representable values so both sides see identical inputs
        P[k] = P[k].float().double()
    return P


CONFIGS = {'one window': (dict(base_filters=4, groups=2, reduction=2, depth=2), (5, 6, 7), 8, (8, 8, 8)),
           '3x1x5 windows': (dict(base_filters=8, groups=2, reduction=2, depth=3), (13, 9, 16), 8, (8, 16, 8))}
MEAN, STD = torch.tensor([95.0, 110.0]), torch.tensor([35.0, 45.0])
FLIPS = [7, 0, 4, 3, 2, 5, 1, 6]     # infer.augment_axes' order; the mean does not depend on it beyond rounding


def volume(vol):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(vol + (2,), generator=g) * 40.0 + 100.0
    mask = (torch.rand(vol + (1,), generator=g) > 0.15).float()
    return x * mask, mask


def engine_model(kw, roi, P):
    from bts_amd.model import Model
    m = Model(**kw)
    if kw.get('data_format') == 'channels_first':
        m(torch.zeros((1, 2) + tuple(roi)))
    else:
        m.build((1,) + tuple(roi) + (2,))
    m.set_weights_from(P)
    return m


def oracle_predict(P, cfg, channels_first=False):
    def predict(win):
        t = torch.from_numpy(np.ascontiguousarray(win)).unsqueeze(0)
        if channels_first:
            return R.model(t.permute(0, 4, 1, 2, 3), P, cfg, training=False, inference=True)[0].permute(0, 2, 3, 4, 1)[0].numpy()
        return R.model(t, P, cfg, training=False, inference=True)[0][0].numpy()
    return predict


@pytest.fixture(scope='module')
def cases():
    """per configuration: volume, parameters (built at the window's extent), the engine's model and the blended fp64 reference
    (computed once, never modified)"""
    import bts_amd  # noqa: F401
    out = {}
    for name, (kw, vol, res, roi) in CONFIGS.items():
        cfg = R.default_config(**kw)
        x, mask = volume(vol)
        xp, mp, orig = R.pad_to_spatial_res(res, x.double(), mask.double())
        P = randomised_params(cfg, roi, seed=5)
        y_ref = WR.sliding_ref(xp.numpy(), mp.numpy(), oracle_predict(P, cfg), roi, FLIPS, MEAN.double().numpy(), STD.double().numpy())
        y_ref = torch.from_numpy(y_ref)[:orig[0], :orig[1], :orig[2]]
        out[name] = dict(kw=kw, vol=vol, res=res, roi=roi, cfg=cfg, x=x, mask=mask, P=P, y_ref=y_ref, model=engine_model(kw, roi, P),
                         padded=tuple(xp.shape[:3]))
    return out


@pytest.mark.parametrize('name', list(CONFIGS))
def test_windowed_segment_volume_matches_oracle(cases, name):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c = cases[name]
    vol, roi = c['vol'], c['roi']
    assert infer.augment_axes(True) == FLIPS
    starts = WR.plan(c['padded'], roi)[0]
    assert [len(s) for s in starts] == ([1, 1, 1] if name == 'one window' else [3, 1, 5])
    spec = infer.WindowSpec(roi, overlap=0.5)
    y, lab = infer.segment_volume(c['model'], c['x'].to(dev()), c['mask'].to(dev()), MEAN, STD, c['res'], window=spec)
    torch.cuda.synchronize()
    assert tuple(y.shape) == vol + (3,) and tuple(lab.shape) == vol and lab.dtype == torch.uint8
    y_ref = c['y_ref']
    err = float((y.double().cpu() - y_ref).abs().max())
    print('%s: max |engine - oracle| = %.3e' % (name, err))
    assert err <= 1e-4, 'windowed TTA probabilities: max abs err %.3e' % err
    lab_ref = R.tta_labels(y_ref, c['mask'].double(), 0.5)
    best = y_ref.max(dim=-1).values
    top2 = torch.topk(y_ref, 2, dim=-1).values
    amb = ((best - 0.5).abs() < 1e-4) | ((top2[..., 0] - top2[..., 1]) < 1e-4)
    bad = (lab.cpu() != lab_ref) & ~amb
    assert int(bad.sum()) == 0, '%d label mismatches outside the ambiguous set (%d ambiguous)' % (int(bad.sum()), int(amb.sum()))
    assert set(lab.cpu().unique().tolist()) <= {0, 1, 2, 4}
    # jobs one by one and three at a time (chunks that span windows, a ragged last chunk)
    outs = [infer.segment_volume(c['model'], c['x'].to(dev()), c['mask'].to(dev()), MEAN, STD, c['res'],
                                 window=infer.WindowSpec(roi, batch=b))[0] for b in (1, 3)]
    assert float((outs[0] - outs[1]).abs().max()) <= 2e-6 and float((outs[0] - y).abs().max()) <= 2e-6


def test_one_constant_window_is_the_whole_volume_path(cases):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c = cases['one window']
    args = (c['model'], c['x'].to(dev()), c['mask'].to(dev()), MEAN, STD, c['res'])
    whole, lab_whole = infer.segment_volume(*args)
    win, lab_win = infer.segment_volume(*args, window=infer.WindowSpec(c['roi'], mode='constant'))
    assert float((whole - win).abs().max()) <= 2e-6
    assert float((lab_whole != lab_win).float().mean()) <= 1e-3


def test_channel_tta_draws_are_those_of_the_whole_volume_path(cases):
    """one 'constant' window over the whole padded volume with two intensity draws per flip: the same generator, the same draws in the
    same order, the deviation of the whole volume -> the unwindowed result within the batching bound"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c = cases['one window']
    xp, mp, _ = infer.pad_to_spatial_res(c['res'], c['x'].to(dev()), c['mask'].to(dev()))
    got = {}
    for name, spec in (('whole', None), ('window', infer.WindowSpec(c['roi'], mode='constant')), ('again', infer.WindowSpec(c['roi'], mode='constant'))):
        tta = infer.TestTimeAugmentor(MEAN, STD, c['model'], channel_tta=2, seed=3, window=spec)
        got[name] = tta(xp, mp)
    plain = infer.TestTimeAugmentor(MEAN, STD, c['model'], window=infer.WindowSpec(c['roi'], mode='constant'))(xp, mp)
    assert float((got['whole'] - got['window']).abs().max()) <= 2e-6
    assert float((got['again'] - got['window']).abs().max()) <= 2e-6
    assert float((plain - got['window']).abs().max()) > 1e-5                     # the draws did move the copies


def test_skipping_empty_windows_changes_nothing(cases):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c = cases['3x1x5 windows']
    x, mask = c['x'].clone(), c['mask'].clone()
    mask[:, :, :8] = 0.0                                                         # the first window along W holds no brain voxel
    x = x * mask
    tta = {}
    for skip in (True, False):
        xp, mp, _ = infer.pad_to_spatial_res(c['res'], x.to(dev()), mask.to(dev()))
        t = infer.TestTimeAugmentor(MEAN, STD, c['model'], window=infer.WindowSpec(c['roi'], skip_empty=skip))
        tta[skip] = (t(xp, mp), t.labels(), t.window_counts)
    assert tta[False][2] == (15, 0)
    run, skipped = tta[True][2]
    assert run + skipped == 15 and skipped >= 3
    assert torch.equal(tta[True][0], tta[False][0]) and torch.equal(tta[True][1], tta[False][1])
    assert float(tta[True][0].abs().max()) > 0.0


def test_channels_first_model_and_the_resolution_check(cases):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c = cases['3x1x5 windows']
    kw = dict(c['kw'], data_format='channels_first')
    cfg = R.default_config(**kw)
    vol, roi = (5, 9, 16), (8, 16, 8)
    x, mask = volume(vol)
    P = randomised_params(cfg, roi, seed=5)
    xp, mp, orig = R.pad_to_spatial_res(8, x.double(), mask.double())
    y_ref = WR.sliding_ref(xp.numpy(), mp.numpy(), oracle_predict(P, cfg, True), roi, [0, 7], MEAN.double().numpy(), STD.double().numpy())
    y_ref = torch.from_numpy(y_ref)[:orig[0], :orig[1], :orig[2]]
    m = engine_model(kw, roi, P)
    tta = infer.TestTimeAugmentor(MEAN, STD, m, 'channels_first', window=infer.WindowSpec(roi))
    tta.flips = [0, 7]
    xg, mg, _ = infer.pad_to_spatial_res(8, x.to(dev()), mask.to(dev()))
    y = tta(xg, mg)
    assert tuple(y.shape) == (3,) + tuple(xp.shape[:3])
    err = float((y.permute(1, 2, 3, 0)[:orig[0], :orig[1], :orig[2]].double().cpu() - y_ref).abs().max())
    assert err <= 1e-4, 'channels_first windowed probabilities: max abs err %.3e' % err
    y, lab = infer.segment_volume(m, x.to(dev()), mask.to(dev()), MEAN, STD, 8, spatial_tta=False, window=infer.WindowSpec(roi))
    assert tuple(y.shape) == (3,) + vol and tuple(lab.shape) == vol
    with pytest.raises(ValueError, match='resolution'):
        infer.segment_volume(m, x.to(dev()), mask.to(dev()), MEAN, STD, 8, window=infer.WindowSpec((8, 12, 8)))


# ---- the command -------------------------------------------------------------------------------------------------------------------
CASE_VOL, CASE_KW, CASE_ROI = (9, 10, 13), dict(base_filters=4, groups=2, reduction=2, depth=2), (8, 8, 8)


def write_case(folder, vol, seed):
    """two modalities with smooth positive texture and a zero slab (background for the brain mask) at the start of the last axis"""
    from bts_amd import nifti
    os.makedirs(folder)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in vol], indexing='ij')
    rng = np.random.default_rng(seed)
    tex = 0.65 + 0.3 * np.sin(5.0 * g[0] + 1.0) * np.cos(4.0 * g[1] + 2.0) * np.sin(6.0 * g[2] + 0.5) + 0.02 * rng.standard_normal(vol)
    tex[:, :, :8] = 0.0
    for name, a in (('c_t1ce.nii.gz', 160.0), ('c_flair.nii', 190.0)):
        nifti.save(os.path.join(folder, name), (tex * a).astype(np.float32), np.eye(4))


def write_model(folder, kw, build, seed):
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    m = Model(**kw)
    m.build((1,) + tuple(build) + (2,))
    m.set_weights_from(randomised_params(R.default_config(**kw), tuple(build), seed))
    save_checkpoint(folder, m)
    save_train_args(folder, {'model_args': dict(kw), 'crop_size': list(build)})


def test_command_with_and_without_window(tmp_path, capsys):
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti
    from bts_amd import test as T
    data = tmp_path / 'data'
    write_case(str(data / 'a'), CASE_VOL, 5)
    write_model(str(tmp_path / 'tumor'), CASE_KW, CASE_ROI, 31)
    np.save(str(tmp_path / 'tp.npy'), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                      'norm': {'mean': np.array([100.0, 120.0]).reshape(1, 1, 1, 2),
                                               'std': np.array([40.0, 50.0]).reshape(1, 1, 1, 2)}})
    base = ['--in_locs', str(data), '--modalities', 't1ce,flair', '--gpu', '--tumor_model', str(tmp_path / 'tumor'),
            '--tumor_prepro', str(tmp_path / 'tp.npy'), '--workers', '0']
    assert T.main(base + ['--out_loc', str(tmp_path / 'plain')]) == 0
    plain = capsys.readouterr().out
    assert 'Windows run' not in plain and '1 cases segmented' in plain
    texts = {}
    for flag in ('8,8,8', 'crop'):
        assert T.main(base + ['--out_loc', str(tmp_path / flag), '--window', flag, '--window_overlap', '0.5']) == 0
        texts[flag] = capsys.readouterr().out
    # padded to (12,12,16): 2 x 2 x 3 windows, the two layers that start at w = 0 lie wholly on the zero slab
    assert 'a. Windows run (skipped as empty): tumor 8 (4)' in texts['8,8,8'] and 'a. Windows run (skipped as empty): tumor 8 (4)' in texts['crop']
    args = T.parse_args(base)
    stage = T.load_stage(str(tmp_path / 'tumor'), str(tmp_path / 'tp.npy'), args, CASE_VOL)
    x, _ = T.upload_case(T.decode_case(str(data / 'a'), ['t1ce', 'flair'], ''), dev())
    _, lab = infer.segment_case(stage, x, (1.0, 1.0, 1.0), window=infer.WindowSpec(CASE_ROI))
    assert stage.window_counts == (8, 4)
    for flag in ('8,8,8', 'crop'):
        got = nifti.load(str(tmp_path / flag / 'a' / 'mask.nii'))[0]
        assert got.shape == CASE_VOL and np.array_equal(got, lab.cpu().numpy())
    assert lab.any()
    # the stage's own WindowSpec does what the argument does, and the plain call is untouched by either
    _, lab_plain = infer.segment_case(stage, x, (1.0, 1.0, 1.0))
    assert np.array_equal(nifti.load(str(tmp_path / 'plain' / 'a' / 'mask.nii'))[0], lab_plain.cpu().numpy())
    own = infer.StageSpec(stage.model, stage.mean, stage.std, stage.spatial_res, window=infer.WindowSpec(CASE_ROI))
    assert torch.equal(infer.segment_case(own, x, (1.0, 1.0, 1.0))[1], lab)
