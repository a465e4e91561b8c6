"""-m gpu: csrc/regions.hip (bts_region_targets, bts_region_dice_sums, bts_region_finish) against the numpy restatement of
tests/regions_ref.py, bit for bit; targets='regions' through prepare_dataset, a training step against the fp64 oracle, whole-volume
inference against the fp64 oracle, and the train and test commands end to end."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import regions_ref as RR  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

# spatial extents of one example: 105 voxels (a tail, odd example offsets), 1 voxel, 10240 and 20480 voxels (several workgroups); STRIDE
# is one voxel more than a whole number of groups beyond what the largest grid takes in one sweep (2048 workgroups x 256 lanes x 4 voxels)
SHAPES = [(3, 5, 7), (1, 1, 1), (16, 16, 40), (16, 32, 40)]
STRIDE = 2048 * 256 * 4 + 4 * 771 + 1


def dev():
    return torch.device('cuda', 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def label_map(rng, shape):
    return np.array([0, 1, 2, 4])[rng.integers(0, 4, size=shape)]


def onehot32(lab):
    return torch.from_numpy(RR.onehot(lab).astype(np.float32))


# ---- bts_region_targets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_first', [False, True])
@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_targets_are_the_encoding_bit_for_bit(shape, n, channels_first):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(sum(shape) + n)
    lab = label_map(rng, (n,) + shape)
    want = torch.from_numpy(RR.encode(RR.onehot(lab)).astype(np.float32))
    y = onehot32(lab)
    if channels_first:
        y, want = y.permute(0, 4, 1, 2, 3).contiguous(), want.permute(0, 4, 1, 2, 3).contiguous()
    yg = y.to(dev())
    out = ops.region_targets(yg, channels_first)
    assert out is yg and torch.equal(bits(yg), bits(want))
    # the round trip on the device: decode(encode(L)) = L
    reg = yg.permute(0, 2, 3, 4, 1).contiguous() if channels_first else yg
    _, back = ops.region_finish(reg, torch.ones((n,) + shape + (1,), device=dev()), 0.5, want_probabilities=False)
    assert np.array_equal(back.cpu().numpy(), lab)


@pytest.mark.parametrize('channels_first', [False, True])
def test_targets_of_a_view_inside_a_larger_buffer(channels_first):
    """the batch starts 12 bytes into its buffer (no 16-byte alignment: the voxel-by-voxel path); the floats on either side stay"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(5)
    n, shape = 2, (16, 16, 40)
    lab = label_map(rng, (n,) + shape)
    y, want = onehot32(lab), torch.from_numpy(RR.encode(RR.onehot(lab)).astype(np.float32))
    if channels_first:
        y, want = y.permute(0, 4, 1, 2, 3).contiguous(), want.permute(0, 4, 1, 2, 3).contiguous()
    buf = torch.full((y.numel() + 11,), 7.25, device=dev())
    view = buf[3:3 + y.numel()].view(y.shape)
    assert view.data_ptr() % 16 == 12 and view.is_contiguous()
    view.copy_(y.to(dev()))
    ops.region_targets(view, channels_first)
    assert torch.equal(bits(view), bits(want))
    assert torch.equal(buf[:3].cpu(), torch.full((3,), 7.25)) and torch.equal(buf[3 + y.numel():].cpu(), torch.full((8,), 7.25))


def test_targets_beyond_one_sweep_of_the_grid():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    rng = np.random.default_rng(6)
    lab = label_map(rng, (1, STRIDE))
    y, want = onehot32(lab), RR.encode(RR.onehot(lab)).astype(np.float32)
    for channels_first in (False, True):
        yg = (y.permute(0, 2, 1).contiguous() if channels_first else y).to(dev())
        ops.region_targets(yg, channels_first)
        got = yg.permute(0, 2, 1) if channels_first else yg
        assert np.array_equal(got.cpu().numpy(), want)


def test_ops_refuse_other_channel_counts():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    d = dev()
    with pytest.raises(ValueError, match='three channels'):
        ops.region_targets(torch.zeros((1, 4, 2), device=d))
    with pytest.raises(ValueError, match='three channels'):
        ops.region_targets(torch.zeros((1, 2, 4), device=d), channels_first=True)
    with pytest.raises(ValueError, match='three channels'):
        ops.region_dice_sums(torch.zeros((1, 2, 2, 2, 4), device=d), torch.zeros((1, 2, 2, 2, 4), device=d))
    with pytest.raises(ValueError, match='three channels'):
        ops.region_finish(torch.zeros((1, 2, 2, 2, 2), device=d), torch.ones((1, 2, 2, 2, 1), device=d))
    with pytest.raises(ValueError, match='dense'):
        ops.region_targets(torch.zeros((1, 4, 6), device=d)[:, :, :3])


# ---- targets='regions' in prepare_dataset --------------------------------------------------------------------------------------------
SIZE = (20, 18, 22, 2)


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    """the dataset of tests/test_train_cli_gpu.py: 5 training and 2 validation examples of 20x18x22x2 with labels 0..3"""
    loc = str(tmp_path_factory.mktemp('regions_dataset'))
    rs = np.random.RandomState(5)
    for sub, n in (('train', 5), ('val', 2)):
        os.makedirs(os.path.join(loc, sub))
        for i in range(n):
            lab = (rs.rand(*SIZE[:3]) * 4).astype(np.int64).astype(np.float32)[..., None]
            np.savez(os.path.join(loc, sub, 'ex%d.npz' % i), x=rs.randn(*SIZE).astype(np.float32), y=lab)
    np.save(os.path.join(loc, 'prepro.npy'), {'size': dict(zip('hwdc', SIZE)), 'norm': {'mean': np.zeros(2), 'std': np.ones(2)}},
            allow_pickle=True)
    return loc


@pytest.mark.parametrize('aug', ['plain', 'spatial', 'spatial+intensity'])
@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
@pytest.mark.parametrize('batched', [False, True])
def test_regions_batches_are_the_encoded_labels_batches(folder, batched, fmt, aug):
    """same seed, the two modes: x and both generator states equal, y of 'regions' = bts_region_targets of y of 'labels', bit for bit"""
    import bts_amd  # noqa: F401
    from bts_amd import data, ops
    extra = {}
    if aug != 'plain':
        extra['spatial'] = data.SpatialConfig(0.7, rotate_deg=20.0, zoom=(0.8, 1.2), elastic_sigma=1.5, elastic_spacing=8)
    if aug == 'spatial+intensity':
        extra['intensity'] = data.IntensityConfig(noise_prob=0.6, blur_prob=0.6, brightness_prob=0.6, contrast_prob=0.6, gamma_prob=0.6)
    sets = {}
    for targets in data.TARGETS:
        sets[targets] = data.prepare_dataset(os.path.join(folder, 'train'), 2, SIZE, (16, 16, 16), 3, shuffle=True, data_format=fmt, seed=3,
                                             device=dev(), rank=0, world=1, resident_bytes=(1 << 30) if batched else 0, workers=0,
                                             targets=targets, **extra)[0]
    cf = fmt == 'channels_first'
    for epoch in range(2):
        got = {k: [(x.clone(), y.clone()) for x, y in ds] for k, ds in sets.items()}
        assert len(got['labels']) == len(got['regions']) == 3
        for (xl, yl), (xr, yr) in zip(got['labels'], got['regions']):
            assert tuple(yr.shape) == ((xl.shape[0], 3, 16, 16, 16) if cf else (xl.shape[0], 16, 16, 16, 3))
            assert torch.equal(bits(xl), bits(xr))
            assert not torch.equal(yl, yr)
            assert torch.equal(bits(ops.region_targets(yl.clone(), cf)), bits(yr))
            reg = (yr.permute(0, 2, 3, 4, 1) if cf else yr).cpu().numpy()
            assert np.all(reg[..., 2] <= reg[..., 1]) and np.all(reg[..., 1] <= reg[..., 0])
        a, b = sets['labels'].state_dict(), sets['regions'].state_dict()
        assert torch.equal(a['gen'], b['gen']) and torch.equal(a['order_gen'], b['order_gen'])


# ---- bts_region_dice_sums --------------------------------------------------------------------------------------------------------------
def dice_inputs(seed, shape, ldt, ldp):
    """-> (t, p) device views (1,)+shape+(3,) with voxel strides ldt, ldp, and their dense host copies.  p: random probabilities, a
    sixth of them exactly 0.5 (not above) and a sixth nextafter(0.5, 1) (above); t: the regions of a random label map"""
    rng = np.random.default_rng(seed)
    full = (1,) + shape
    p = rng.random(full + (3,)).astype(np.float32)
    pick = rng.integers(0, 6, size=p.shape)
    p[pick == 0] = np.float32(0.5)
    p[pick == 1] = np.nextafter(np.float32(0.5), np.float32(1.0))
    t = RR.encode(RR.onehot(label_map(rng, full))).astype(np.float32)
    out = []
    for a, ld in ((t, ldt), (p, ldp)):
        if ld == 3:
            out.append(torch.from_numpy(a).to(dev()))
        else:
            buf = torch.full(full + (ld,), 0.75, device=dev())          # 0.75 > 0.5: a read of the padding would be counted
            v = buf[..., 1:4]
            v.copy_(torch.from_numpy(a).to(dev()))
            out.append(v)
    return out[0], out[1], t, p


def coded(lab):
    """regions_ref's {0,1,2,4} map in the coding of .last_labels: 3 for ET"""
    return np.where(lab == 4, 3, lab).astype(np.uint8)


@pytest.mark.parametrize('ldt,ldp', [(3, 3), (3, 8), (8, 3), (8, 8)])
@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 5, 7), (16, 32, 40)])
def test_dice_sums_are_the_counts(shape, ldt, ldp):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    tg, pg, t, p = dice_inputs(sum(shape), shape, ldt, ldp)
    if np.prod(shape) > 1:
        assert ops.ld_of(tg) == ldt and ops.ld_of(pg) == ldp
    table, labels = ops.region_dice_sums(tg, pg)
    want = RR.dice_counts(t, p)
    got = table.cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float64))
    assert labels.dtype == torch.uint8 and np.array_equal(labels.cpu().numpy(), coded(RR.decode(p, None, np.float32(0.5), strict=True)))
    if np.prod(shape) > 100:
        assert want.min() > 0 and (p == np.float32(0.5)).sum() > 10
    table2, none = ops.region_dice_sums(tg, pg, want_labels=False)
    assert none is None and torch.equal(table.view(torch.int64), table2.view(torch.int64))


def test_dice_sums_overwrite_their_outputs_and_run_past_one_sweep():
    """the C ABI on buffers full of 0xFF, at a size beyond one sweep of the grid and off 4-voxel groups"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    from bts_amd._lib import lib
    nv = STRIDE // 2 + 2                                               # the Dice grid is half the streaming one: 1024 workgroups
    tg, pg, t, p = dice_inputs(9, (1, 1, nv), 3, 3)
    table = torch.full((9,), float('nan'), dtype=torch.float64, device=dev())
    table.view(torch.uint8).fill_(255)
    labels = torch.full((nv,), 255, dtype=torch.uint8, device=dev())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    for _ in range(2):
        lib().call('bts_region_dice_sums', ptr(tg), ptr(pg), ptr(labels), ptr(table), nv, 3, 3, 3, stream)
    assert np.array_equal(table.cpu().numpy(), RR.dice_counts(t, p).astype(np.float64))
    want = coded(RR.decode(p, None, np.float32(0.5), strict=True)).reshape(-1)
    assert np.array_equal(labels.cpu().numpy(), want) and int(labels.max()) == 3


@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
def test_region_dice_coefficient(fmt):
    import bts_amd  # noqa: F401
    from bts_amd.util import RegionDiceCoefficient
    rng = np.random.default_rng(17)
    shape = (2, 6, 5, 9)
    p = rng.random(shape + (3,)).astype(np.float32)
    t = RR.encode(RR.onehot(label_map(rng, shape))).astype(np.float32)
    tg, pg = torch.from_numpy(t).to(dev()), torch.from_numpy(p).to(dev())
    if fmt == 'channels_first':
        tg, pg = tg.permute(0, 4, 1, 2, 3).contiguous(), pg.permute(0, 4, 1, 2, 3).contiguous()
    fn = RegionDiceCoefficient(data_format=fmt)
    assert fn.name == 'region_dice' and fn.last_labels is None
    macro, micro = fn(tg, pg)
    want = RR.dice_value(RR.dice_counts(t, p))
    assert tuple(macro.shape) == (1,) and tuple(micro.shape) == (1,)
    # float32 output of a float64 computation
    assert abs(float(macro) - want[0]) <= 1e-6 * want[0] and abs(float(micro) - want[1]) <= 1e-6 * want[1]
    assert np.array_equal(fn.last_labels.cpu().numpy(), coded(RR.decode(p, None, np.float32(0.5), strict=True)))
    with pytest.raises(ValueError):
        RegionDiceCoefficient(data_format='NCDHW')


# ---- bts_region_finish -----------------------------------------------------------------------------------------------------------------
def finish_inputs(seed, shape, threshold):
    rng = np.random.default_rng(seed)
    p = rng.random(shape + (3,)).astype(np.float32)
    pick = rng.integers(0, 8, size=p.shape)
    p[pick == 0] = np.float32(threshold)                               # exactly at the threshold: passes (>=)
    p[pick == 1] = np.nextafter(np.float32(threshold), np.float32(0.0))
    m = (rng.random(shape + (1,)) > 0.3).astype(np.float32)
    return p, m


@pytest.mark.parametrize('threshold', [0.5, 0.3])
@pytest.mark.parametrize('shape', [(2, 5, 6, 7), (1, 1, 1, 1), (1, 16, 32, 40)])
def test_finish_masks_and_decodes(shape, threshold):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    p, m = finish_inputs(sum(shape), shape, threshold)
    want = RR.decode(p, m, np.float32(threshold))
    y, lab = ops.region_finish(torch.from_numpy(p).to(dev()), torch.from_numpy(m).to(dev()), threshold)
    assert torch.equal(bits(y), bits(torch.from_numpy(p * m)))
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == shape and np.array_equal(lab.cpu().numpy(), want)
    assert set(np.unique(lab.cpu().numpy()).tolist()) <= {0, 1, 2, 4}
    if np.prod(shape) > 100:
        assert set(np.unique(want).tolist()) == {0, 1, 2, 4} and (want != RR.decode_nested(p * m, np.float32(threshold))).any()
    # either output alone, and prob as a view 12 bytes into a larger buffer (the voxel-by-voxel path)
    y2, none = ops.region_finish(torch.from_numpy(p).to(dev()), torch.from_numpy(m).to(dev()), threshold, want_labels=False)
    assert none is None and torch.equal(y2, y)
    buf = torch.zeros(p.size + 5, device=dev())
    view = buf[3:3 + p.size].view(p.shape)
    view.copy_(torch.from_numpy(p))
    none, lab3 = ops.region_finish(view, torch.from_numpy(m).to(dev()), threshold, want_probabilities=False)
    assert none is None and torch.equal(lab3, lab)


def test_finish_overwrites_its_outputs_and_runs_past_one_sweep():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    nv = STRIDE
    p, m = finish_inputs(4, (nv,), 0.5)
    pg, mg = torch.from_numpy(p).to(dev()), torch.from_numpy(m).to(dev())
    y = torch.empty_like(pg)
    y.view(torch.uint8).fill_(255)
    lab = torch.full((nv,), 255, dtype=torch.uint8, device=dev())
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    lib().call('bts_region_finish', ptr(pg), ptr(mg), ptr(y), ptr(lab), nv, 3, 0.5, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(y.cpu().numpy(), p * m)
    assert np.array_equal(lab.cpu().numpy(), RR.decode(p, m, np.float32(0.5)))


# ---- a training step on region targets against the fp64 oracle ---------------------------------------------------------------------------
def test_train_step_on_region_targets_matches_the_oracle():
    """smoke()'s set-up with y region-encoded on both sides: nothing in the loss or its backward assumes disjoint targets"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    from bts_amd.model import Model
    from bts_amd.tape import as_tensor
    from bts_amd.util import DiceVAELoss, RegionDiceCoefficient, ScheduledOptim, train_step
    kw = dict(base_filters=8, groups=4, reduction=2, depth=3)
    crop, n = (16, 16, 16), 1
    cfg = R.default_config(**kw)
    x, y, mask, eps = R.synthetic_batch(n, crop, latent=cfg['base_filters'] * 2 ** (cfg['depth'] - 2), seed=1234)
    y_reg = torch.from_numpy(RR.encode(y.numpy()).astype(np.float32))
    assert float((y_reg - y).abs().sum()) > 0 and set(y_reg.unique().tolist()) == {0.0, 1.0}
    assert torch.equal(ops.region_targets(y.to(dev())).cpu(), y_reg)
    P = R.build_params(cfg, crop, seed=3)
    g = torch.Generator().manual_seed(5)
    for k in P:
        if k.endswith('gn2_g'):
            P[k] = torch.randn(P[k].shape, generator=g, dtype=torch.float64)
        P[k] = P[k].float().double()
    model = Model(**kw)
    model.build((n,) + crop + (2,))
    model.set_weights_from(P)
    model.encoder.set_dropout_mask(mask)
    model.vae.set_eps(eps)
    opt = ScheduledOptim(1e-4)
    opt(epoch=0)

    class Keeping(RegionDiceCoefficient):
        def __call__(self, y_true, y_pred):
            self.y_pred = as_tensor(y_pred, data_format=self.data_format).t.detach().clone()
            return RegionDiceCoefficient.__call__(self, y_true, y_pred)

    dice_fn = Keeping()
    loss, macro, micro = train_step(model, opt, DiceVAELoss(), dice_fn, x, y_reg)
    torch.cuda.synchronize()
    state = {}
    loss_r, _, _, _, outs = R.train_step(P, cfg, x.double(), y_reg.double(), mask.double(), eps.double(), state, 1e-4, 1)
    print('loss %.7f, oracle %.7f' % (float(loss), float(loss_r)))
    assert abs(float(loss) - float(loss_r)) < 1e-5 * max(1.0, abs(float(loss_r))), (float(loss), float(loss_r))
    worst = 0.0
    for p in model.trainable_variables:
        worst = max(worst, float((p.t.cpu().double() - P[model.oracle_name(p)]).abs().max()))
    print('max |param - oracle| after Adam %.3e' % worst)
    assert worst < 5e-6, worst
    yp = dice_fn.y_pred.cpu().numpy()
    assert yp.shape == (n,) + crop + (3,) and float(np.abs(yp - outs[0].numpy()).max()) < 1e-4
    want = RR.dice_value(RR.dice_counts(y_reg.numpy(), yp))
    assert abs(float(macro) - want[0]) <= 1e-6 * want[0] and abs(float(micro) - want[1]) <= 1e-6 * abs(want[1])
    assert np.array_equal(dice_fn.last_labels.cpu().numpy(), coded(RR.decode(yp, None, np.float32(0.5), strict=True)))


# ---- whole-volume inference against the fp64 oracle ------------------------------------------------------------------------------------------
CONFIGS = [(dict(base_filters=4, groups=2, reduction=2, depth=2), (5, 6, 7), 8), (dict(base_filters=8, groups=2, reduction=2, depth=3), (13, 9, 16), 8)]
MEAN, STD = torch.tensor([95.0, 110.0]), torch.tensor([35.0, 45.0])


def randomised_params(cfg, crop, seed):
    """tests/test_infer_gpu.py's: the oracle ParamSet with every gamma / beta / bias randomised, fp32-representable"""
    P = R.build_params(cfg, crop, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in P:
        if k.endswith('_b'):
            P[k] = torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.1
        if k.endswith('_g'):
            P[k] = 1.0 + torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.3
    for k in P:
        P[k] = P[k].float().double()
    return P


@pytest.fixture(scope='module')
def volumes():
    """per configuration of tests/test_infer_gpu.py::test_segment_volume_matches_oracle: volume, mask, the engine's model and the
    oracle's masked mean probabilities with their decoded map (computed once, never modified)"""
    import bts_amd  # noqa: F401
    from bts_amd.model import Model
    out = []
    for kw, vol, res in CONFIGS:
        cfg = R.default_config(**kw)
        g = torch.Generator().manual_seed(21)
        x = torch.randn(vol + (2,), generator=g) * 40.0 + 100.0
        mask = (torch.rand(vol + (1,), generator=g) > 0.15).float()
        x = x * mask
        xp, mp, orig = R.pad_to_spatial_res(res, x.double(), mask.double())
        P = randomised_params(cfg, tuple(xp.shape[:3]), seed=5)
        y_ref = R.tta_predict(xp, mp, P, cfg, MEAN.double(), STD.double())[:orig[0], :orig[1], :orig[2]].numpy()
        m = Model(**kw)
        m.build((1,) + tuple(xp.shape[:3]) + (2,))
        m.set_weights_from(P)
        amb = (np.abs(y_ref - 0.5) < 1e-4).any(axis=-1)
        out.append(dict(vol=vol, res=res, x=x, mask=mask, model=m, padded=tuple(xp.shape[:3]), y_ref=y_ref, amb=amb,
                        lab_ref=RR.decode(y_ref, mask.numpy().astype(np.float64), 0.5)))
    return out


def same_map(lab, c):
    lab = lab.cpu().numpy()
    assert lab.dtype == np.uint8 and lab.shape == c['vol'] and set(np.unique(lab).tolist()) <= {0, 1, 2, 4}
    bad = (lab != c['lab_ref']) & ~c['amb']
    assert int(bad.sum()) == 0, '%d label mismatches outside the ambiguous set (%d ambiguous)' % (int(bad.sum()), int(c['amb'].sum()))


@pytest.mark.parametrize('which', [0, 1])
def test_segment_volume_with_region_targets_matches_oracle(volumes, which):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    c = volumes[which]
    vol, res = c['vol'], c['res']
    assert c['amb'].mean() <= 0.01, 'ambiguous set: %d of %d voxels' % (int(c['amb'].sum()), c['amb'].size)
    if which == 0:
        assert set(np.unique(c['lab_ref']).tolist()) == {0, 1, 2, 4}
    assert (c['lab_ref'] != RR.decode_nested(c['y_ref'], 0.5)).any()                   # the two rules can be told apart here
    xg, mg = c['x'].to(dev()), c['mask'].to(dev())
    y, lab = infer.segment_volume(c['model'], xg, mg, MEAN, STD, res, targets='regions')
    torch.cuda.synchronize()
    assert tuple(y.shape) == vol + (3,)
    err = float(np.abs(y.double().cpu().numpy() - c['y_ref']).max())
    print('max |engine - oracle| = %.3e, %d ambiguous voxels of %d' % (err, int(c['amb'].sum()), c['amb'].size))
    assert err <= 1e-4, 'TTA probabilities: max abs err %.3e' % err
    same_map(lab, c)
    # the probabilities do not depend on the mode, the map does
    y0, lab0 = infer.segment_volume(c['model'], xg, mg, MEAN, STD, res)
    assert torch.equal(y0, y) and not torch.equal(lab0, lab)
    # the augmented copies three at a time
    yb, labb = infer.segment_volume(c['model'], xg, mg, MEAN, STD, res, tta_batch=3, targets='regions')
    assert float((yb - y).abs().max()) <= 2e-6
    same_map(labb, c)
    # through segment_scan on the scan's own grid: its brain mask (any channel > 0) is this volume's
    assert torch.equal((c['x'].max(dim=-1, keepdim=True).values > 0).float(), c['mask'])
    ys, labs = infer.segment_scan(c['model'], xg, (1.0, 1.0, 1.0), MEAN, STD, res, targets='regions')
    assert float(np.abs(ys.double().cpu().numpy() - c['y_ref']).max()) <= 1e-4
    same_map(labs, c)
    if which == 0:
        # one 8x8x8 window is the padded volume
        assert c['padded'] == (8, 8, 8)
        yw, labw = infer.segment_volume(c['model'], xg, mg, MEAN, STD, res, window=infer.WindowSpec(roi=(8, 8, 8)), targets='regions')
        errw = float(np.abs(yw.double().cpu().numpy() - c['y_ref']).max())
        assert errw <= 1e-4, 'windowed TTA probabilities: max abs err %.3e' % errw
        same_map(labw, c)
        # a resampled scan: (5,6,7) at pixdim (1.2, 1.0, 0.9) is (6,6,6) at 1 mm^3, padded to the same (8,8,8)
        assert infer.zoom_output_shape(vol, (1.2, 1.0, 0.9)) == (6, 6, 6)
        yz, labz = infer.segment_scan(c['model'], xg, (1.2, 1.0, 0.9), MEAN, STD, res, targets='regions')
        assert tuple(yz.shape) == vol + (3,) and tuple(labz.shape) == vol and labz.dtype == torch.uint8
        assert set(np.unique(labz.cpu().numpy()).tolist()) <= {0, 1, 2, 4}
        # ... decoded from the probabilities it returns, on the native grid
        want = RR.decode(yz.cpu().numpy(), None, np.float32(0.5))
        assert np.array_equal(labz.cpu().numpy(), want)


def test_regions_need_a_three_channel_model(volumes):
    import bts_amd  # noqa: F401
    from bts_amd import infer
    from bts_amd.model import Model
    m = Model(base_filters=4, groups=2, reduction=2, depth=2, out_ch=2)
    m.build((1, 8, 8, 8, 2))
    c = volumes[0]
    with pytest.raises(ValueError, match='out_ch = 2'):
        infer.segment_volume(m, c['x'].to(dev()), c['mask'].to(dev()), MEAN, STD, 8, targets='regions')
    with pytest.raises(ValueError, match='unknown targets'):
        infer.segment_volume(c['model'], c['x'].to(dev()), c['mask'].to(dev()), MEAN, STD, 8, targets='nested')


# ---- the commands end to end ---------------------------------------------------------------------------------------------------------------
MODEL_FLAGS = ['--crop_size', '16,16,16', '--base_filters', '16', '--groups', '4', '--reduction', '4', '--depth', '3', '--batch_size', '2']
NAMES = ('train_loss', 'train_macro_dice', 'train_micro_dice', 'val_loss', 'val_macro_dice', 'val_micro_dice')
CASE_VOL = (9, 10, 13)


def _argv(folder, out, *more):
    return ['--train_loc', os.path.join(folder, 'train'), '--val_loc', os.path.join(folder, 'val'), '--prepro_loc',
            os.path.join(folder, 'prepro.npy'), '--save_folder', out] + MODEL_FLAGS + list(more)


def _train(argv):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    from bts_amd.layers import _base
    _base.set_seed(0)
    return T, T.run(T.parse_args(argv))


def _log_is_finite(T, out, rows):
    lines = open(os.path.join(out, 'train.log')).read().strip().split('\n')
    assert lines[0] == T.LOG_HEADER and len(lines) == rows + 1
    for ln in lines[1:]:
        vals = [float(v) for v in ln.split(',')]
        assert len(vals) == 8 and np.isfinite(vals[2:]).all(), ln
        assert all(0.0 <= v <= 1.0 for v in (vals[3], vals[4], vals[6], vals[7])), ln


@pytest.fixture(scope='module')
def trained(folder, tmp_path_factory):
    """`python -m bts_amd.train --targets regions --n_epochs 2` in float32 on the small dataset -> (train module, folder, result)"""
    out = os.path.join(str(tmp_path_factory.mktemp('regions_run')), 'run')
    T, res = _train(_argv(folder, out, '--n_epochs', '2', '--data_format', 'channels_last', '--patience', '5', '--targets', 'regions'))
    return T, out, res


def test_train_command_in_float32_and_a_resumed_run(folder, trained):
    from bts_amd.util import RegionDiceCoefficient
    T, out, res = trained
    _log_is_finite(T, out, 2)
    assert T.load_train_args(out)['targets'] == 'regions' and len(res['history']) == 2
    _, meta = T.read_container(os.path.join(out, T.CHECKPOINT_NAME))
    argv = ['--train_loc', os.path.join(folder, 'train'), '--val_loc', os.path.join(folder, 'val'), '--prepro_loc',
            os.path.join(folder, 'prepro.npy'), '--load_folder', out, '--batch_size', '2', '--n_epochs', '3', '--patience', '5',
            '--targets', 'labels']
    args = T.parse_args(argv)
    assert args.targets == 'regions'
    seen = []
    real = T.fit

    def spy(model, optimizer, loss_fn, dice_fn, train_data, val_data, *a, **k):
        seen.append((type(dice_fn), train_data.targets, val_data.targets))
        return real(model, optimizer, loss_fn, dice_fn, train_data, val_data, *a, **k)
    T.fit = spy
    try:
        res2 = T.run(args)
    finally:
        T.fit = real
    assert seen == [(RegionDiceCoefficient, 'regions', 'regions')]
    assert [h['epoch'] for h in res2['history']] == list(range(meta['next_epoch'], 3))
    assert all(np.isfinite([float(h[k]) for k in NAMES]).all() for h in res2['history'])
    assert T.load_train_args(out)['targets'] == 'regions'


def test_train_command_in_bfloat16(folder, tmp_path):
    out = os.path.join(str(tmp_path), 'run16')
    T, res = _train(_argv(folder, out, '--n_epochs', '2', '--data_format', 'channels_first', '--dtype', 'bfloat16', '--targets', 'regions'))
    _log_is_finite(T, out, 2)
    assert T.load_train_args(out)['targets'] == 'regions'
    assert os.path.exists(os.path.join(out, T.CHECKPOINT_NAME))


def write_case(path, vol, seed):
    """tests/test_window_gpu.py's: two modalities with smooth positive texture and a zero slab at the start of the last axis"""
    from bts_amd import nifti
    os.makedirs(path)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in vol], indexing='ij')
    rng = np.random.default_rng(seed)
    tex = 0.65 + 0.3 * np.sin(5.0 * g[0] + 1.0) * np.cos(4.0 * g[1] + 2.0) * np.sin(6.0 * g[2] + 0.5) + 0.02 * rng.standard_normal(vol)
    tex[:, :, :3] = 0.0
    for name, a in (('c_t1ce.nii.gz', 1.6), ('c_flair.nii', 1.9)):
        nifti.save(os.path.join(path, name), (tex * a).astype(np.float32), np.eye(4))


def test_test_command_decodes_by_the_recorded_mode(folder, trained, tmp_path, capsys):
    import shutil
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti
    from bts_amd import test as C
    T, run, _ = trained
    data = tmp_path / 'cases'
    write_case(str(data / 'a'), CASE_VOL, 5)
    prepro = os.path.join(folder, 'prepro.npy')
    masks, stages = {}, {}
    for mode in ('regions', 'labels'):
        model = str(tmp_path / ('model_' + mode))
        shutil.copytree(run, model)
        if mode == 'labels':                                           # the same checkpoint, the key gone: a folder from before the flag
            targs = T.load_train_args(model)
            del targs['targets']
            with open(os.path.join(model, T.ARGS_NAME), 'wb') as f:
                pickle.dump(targs, f)
        base = ['--in_locs', str(data), '--modalities', 't1ce,flair', '--gpu', '--tumor_model', model, '--tumor_prepro', prepro, '--workers', '0']
        assert C.main(base + ['--out_loc', str(tmp_path / mode)]) == 0
        assert '1 cases segmented' in capsys.readouterr().out
        masks[mode] = nifti.load(str(tmp_path / mode / 'a' / 'mask.nii'))[0]
        assert masks[mode].shape == CASE_VOL and set(np.unique(masks[mode]).tolist()) <= {0, 1, 2, 4}
        stages[mode] = C.load_stage(model, prepro, C.parse_args(base), CASE_VOL)
        assert stages[mode].targets == mode
    x, _ = C.upload_case(C.decode_case(str(data / 'a'), ['t1ce', 'flair'], ''), dev())
    st = stages['regions']
    for mode in ('regions', 'labels'):
        own = infer.StageSpec(st.model, st.mean, st.std, st.spatial_res, targets=mode)
        prob, lab = infer.segment_case(own, x, (1.0, 1.0, 1.0))
        assert np.array_equal(masks[mode], lab.cpu().numpy())
        if mode == 'regions':
            assert np.array_equal(masks[mode], RR.decode(prob.cpu().numpy(), None, np.float32(0.5)))
    # today's behaviour for the folder without the key: the arg-max map of the default StageSpec
    _, lab = infer.segment_case(infer.StageSpec(st.model, st.mean, st.std, st.spatial_res), x, (1.0, 1.0, 1.0))
    assert np.array_equal(masks['labels'], lab.cpu().numpy())
