"""-m gpu: the compound loss -- csrc/loss_ce.hip (bts_seg_loss_sums, bts_seg_loss_value, bts_seg_loss_bwd) against the fp64 reference of
tests/loss_ce_ref.py with its bounds and K unchanged, at the edges of tests/test_step_kernels_gpu.py's loss tests (C = 1, 3, 8, channel
slices of sentinel slabs, no VAE operands, past both grid caps) and at the clamp; agreement with the Dice kernels; shard additivity;
util.CompoundVAELoss and LowPrecisionTrainer(loss=...) in one step each; the train command with --loss.  Each check prints its measured
ratio before it asserts (pytest -s).  No test passes a pointer or an extent that lets a kernel touch memory outside its buffers."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import loss_ce_ref as L  # noqa: E402
import step_ref as S  # noqa: E402

SENTINEL = 7.0


def dev():
    return torch.device('cuda:0')


def ops_():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops


def on_slab(t, off, extra=8):
    """t (..., C) -> (slab on the device filled with the sentinel, its view [..., off:off+C] holding t)"""
    c = t.shape[-1]
    slab = torch.full(t.shape[:-1] + (c + extra,), SENTINEL, dtype=t.dtype, device=dev())
    view = slab[..., off:off + c]
    view.copy_(t)
    return slab, view


def sentinel_intact(slab, off, c):
    rest = torch.cat([slab[..., :off], slab[..., off + c:]], -1)
    return bool((rest == SENTINEL).all())


def run_seg(tensors, gs, ts, gamma, alpha, w_dice=1.0, w_ce=1.0, sums=None):
    """tensors: device views (p, y, x, yv, proj) or (p, y, None, None, None) -> sums, value, parts, dlogit, dyvae, dproj"""
    ops = ops_()
    p, y, x, yv, proj = tensors
    c = p.shape[-1]
    g, wp, wn = L.weights(gamma, alpha)
    if sums is None:
        sums = ops.seg_loss_sums(p, y, x, yv, proj, g, wp, wn)
    val, parts = ops.seg_loss_value(sums, c, x is not None, w_dice, w_ce)
    gsc = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=dev())
    dl = torch.full(p.shape, SENTINEL, device=dev())
    dyv = torch.full(x.shape, SENTINEL, device=dev()) if x is not None else None
    dpr = torch.full(proj.shape, SENTINEL, device=dev()) if x is not None else None
    ops.seg_loss_bwd(p, y, x, yv, proj, sums, gsc, dl, dyv, dpr, bool(ts), w_dice, w_ce, g, wp, wn)
    return sums.cpu(), float(val), parts.cpu(), dl, dyv, dpr


def check_seg(out, ref, c, what, vae=True, dice_sums=None):
    sums, val, parts, dl, dyv, dpr = out
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (4 * c + 5,) and bool(torch.isfinite(sums).all())
    for k, name in enumerate('IPT'):
        S.check(sums[k * c:(k + 1) * c], ref[name], S.EPS32 * ref[name], 1.0, what + ' sums ' + name)
    if dice_sums is not None:      # fp64 sums of the same fp32 terms as bts_loss_sums
        a, b = sums[:3 * c + 4], dice_sums.cpu()
        assert bool(((a - b).abs() <= 1e-12 * b.abs()).all()), (a, b)
    S.check(sums[3 * c + 4:4 * c + 4], ref['ce_sums'], ref['B_ce_sums'], L.K_CE_SUM, what + ' CE sums')
    assert float(sums[4 * c + 4]) == ref['count']
    print('%s value: err %.3e, bound %.3e' % (what, abs(val - ref['loss']), ref['value_bound']))
    assert abs(val - ref['loss']) <= ref['value_bound']
    assert abs(float(parts[0]) - ref['dice']) <= 4 * S.EPS32
    assert abs(float(parts[3]) - ref['ce']) <= L.K_CE_SUM * float(ref['B_ce_sums'].sum()) / (ref['count'] * c) + S.EPS32 * ref['ce']
    S.check(dl, ref['dlogit'], ref['B_dlogit'], L.K_CE_GRAD, what + ' dlogit')
    if vae:
        assert float(sums[3 * c + 2]) == ref['numel_x'] and float(sums[3 * c + 3]) == ref['numel_z']
        assert abs(float(sums[3 * c]) - ref['sq']) <= 4 * S.EPS32 * ref['sq']
        assert abs(float(sums[3 * c + 1]) - ref['klsum']) <= 4 * S.EPS32 * ref['klabs']
        assert abs(float(parts[1]) - ref['l2']) <= 4 * S.EPS32 * ref['l2']
        assert abs(float(parts[2]) - ref['kl']) <= 4 * S.EPS32 * ref['klabs'] / ref['numel_z']
        S.check(dyv, ref['dyvae'], ref['B_dyvae'], S.K_LOSS_GRAD, what + ' dyvae')
        S.check(dpr, ref['dproj'], ref['B_dproj'], S.K_LOSS_GRAD, what + ' dproj')
    else:
        assert float(parts[1]) == 0.0 and float(parts[2]) == 0.0


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gamma,alpha', L.CASES)
@pytest.mark.parametrize('shape', L.LOSS_SHAPES_SMALL)
@pytest.mark.parametrize('ts', [1, 0])
@pytest.mark.parametrize('gs', [None, 0.125, 65536.0])
def test_seg_loss_small(shape, ts, gs, gamma, alpha):
    ops = ops_()
    n, dims, c, cx, lz = shape
    host = L.loss_inputs(n, dims, c, cx, lz)
    kw = dict(gs=1.0 if gs is None else gs, through_sigmoid=ts, gamma=gamma, alpha=alpha, w_dice=0.75, w_ce=1.5)
    ref = L.seg_loss_ref(*host, **kw)
    dense = [t.to(dev()) for t in host]
    check_seg(run_seg(dense, gs, ts, gamma, alpha, 0.75, 1.5), ref, c, 'dense', dice_sums=ops.loss_sums(*dense))
    for off in (0, 5):      # y_pred, y, x, y_vae as channel slices of wider slabs
        slabs = [on_slab(t, off) for t in host[:4]]
        check_seg(run_seg([v for _, v in slabs] + [dense[4]], gs, ts, gamma, alpha, 0.75, 1.5), ref, c, 'slice at %d' % off)
        for (sl, v) in slabs:
            assert sentinel_intact(sl, off, v.shape[-1])
    # without the VAE operands
    ref0 = L.seg_loss_ref(host[0], host[1], **kw)
    check_seg(run_seg([dense[0], dense[1], None, None, None], gs, ts, gamma, alpha, 0.75, 1.5), ref0, c, 'no vae', vae=False)


@pytest.mark.parametrize('shape', [L.LOSS_SHAPE_PAST_PARTIAL, L.LOSS_SHAPE_PAST_BWD], ids=['past_sums_cap', 'past_bwd_cap'])
def test_seg_loss_past_the_grid_caps(shape):
    """262,144 voxels fill the 1024 blocks of the sums pass, 1,048,576 the 4096 of the backward: the second trip of each grid-stride loop"""
    n, dims, c, cx, lz = shape
    assert n * dims[0] * dims[1] * dims[2] > (1024 * 256 if shape is L.LOSS_SHAPE_PAST_PARTIAL else 4096 * 256)
    host = L.loss_inputs(n, dims, c, cx, lz)
    ref = L.seg_loss_ref(*host, gs=1.0, through_sigmoid=1, gamma=2.0, alpha=0.25)
    check_seg(run_seg([t.to(dev()) for t in host], None, 1, 2.0, 0.25), ref, c, 'large')


@pytest.mark.parametrize('gamma,alpha', L.CASES)
@pytest.mark.parametrize('ts', [1, 0])
def test_saturation(ts, gamma, alpha):
    """p exactly 0, EPS/2, EPS, 1-EPS, 1-EPS/2, 1 against t = 0 and 1: nothing is NaN or Inf, the cross-entropy gradient is zero strictly
    outside the clamp and the reference's on it"""
    p, t = L.saturation_inputs()
    c = p.shape[-1]
    tensors = [p.to(dev()), t.to(dev()), None, None, None]
    ref = L.seg_loss_ref(p, t, through_sigmoid=ts, gamma=gamma, alpha=alpha)
    out = run_seg(tensors, None, ts, gamma, alpha)
    assert bool(torch.isfinite(out[0]).all()) and np.isfinite(out[1]) and bool(torch.isfinite(out[2]).all())
    assert bool(torch.isfinite(out[3]).all())
    check_seg(out, ref, c, 'saturated', vae=False)
    # the cross-entropy part alone: w_dice = 0
    ref_ce = L.seg_loss_ref(p, t, through_sigmoid=ts, gamma=gamma, alpha=alpha, w_dice=0.0)
    dl = run_seg(tensors, None, ts, gamma, alpha, 0.0, 1.0)[3].cpu()
    outside = (p < L.EPS) | (p > 1.0 - L.EPS)
    assert int(outside.sum()) == p.numel() * 4 // 6 and bool((dl[outside] == 0).all())
    S.check(dl, ref_ce['dlogit'], ref_ce['B_dlogit'], L.K_CE_GRAD, 'saturated CE gradient')
    wrong = ((p.double() == L.EPS) & (t == 1)) | ((p.double() == 1.0 - L.EPS) & (t == 0))
    assert bool((dl[wrong] != 0).all()) and bool((ref_ce['dlogit'][wrong] != 0).all())


def test_soft_targets():
    n, dims, c, cx, lz = L.LOSS_SHAPES_SMALL[0]
    host = list(L.loss_inputs(n, dims, c, cx, lz))
    host[1] = L.soft_targets(host[1].shape)
    assert set(host[1].unique().tolist()) == {0.0, 0.25, 1.0}
    for ts in (1, 0):
        ref = L.seg_loss_ref(*host, through_sigmoid=ts, gamma=2.0, alpha=0.25)
        check_seg(run_seg([t.to(dev()) for t in host], None, ts, 2.0, 0.25), ref, c, 'soft targets')


@pytest.mark.parametrize('shape', L.LOSS_SHAPES_SMALL)
def test_agreement_with_the_dice_kernels(shape):
    """entries [0, 3C+4) are bts_loss_sums'; with w_ce = 0, w_dice = 1 value and dlogit meet step_ref.loss_ref's bounds"""
    ops = ops_()
    n, dims, c, cx, lz = shape
    host = L.loss_inputs(n, dims, c, cx, lz)
    dense = [t.to(dev()) for t in host]
    want = ops.loss_sums(*dense).cpu()
    for ts in (1, 0):
        ref = S.loss_ref(*host, gs=1.0, through_sigmoid=ts)
        for gamma, alpha in L.CASES:
            sums, val, parts, dl, dyv, dpr = run_seg(dense, None, ts, gamma, alpha, 1.0, 0.0)
            assert bool(((sums[:3 * c + 4] - want).abs() <= 1e-12 * want.abs()).all())
            assert abs(val - ref['loss']) <= ref['value_bound']
            S.check(dl, ref['dlogit'], ref['B_dlogit'], S.K_LOSS_GRAD, 'w_ce = 0 dlogit')
            S.check(dyv, ref['dyvae'], ref['B_dyvae'], S.K_LOSS_GRAD, 'w_ce = 0 dyvae')
            S.check(dpr, ref['dproj'], ref['B_dproj'], S.K_LOSS_GRAD, 'w_ce = 0 dproj')


@pytest.mark.parametrize('shape', L.LOSS_SHAPES_SMALL)
def test_seg_loss_shard_additivity(shape):
    """the data-parallel contract of the header: the raw sums of two shards (the voxel count among them) add up to the batch's; each
    shard's gradient rows follow from the summed sums"""
    ops = ops_()
    n, dims, c, cx, lz = shape
    host = L.loss_inputs(n, dims, c, cx, lz)
    gamma, alpha = 2.0, 0.25
    g, wp, wn = L.weights(gamma, alpha)
    ref = L.seg_loss_ref(*host, gs=1.0, through_sigmoid=1, gamma=gamma, alpha=alpha)
    parts = [[t[:1].contiguous().to(dev()) for t in host], [t[1:].contiguous().to(dev()) for t in host]]
    each = [ops.seg_loss_sums(*sh, g, wp, wn) for sh in parts]
    sums = each[0] + each[1]
    whole = ops.seg_loss_sums(*[t.to(dev()) for t in host], g, wp, wn)
    assert float(sums[4 * c + 4]) == ref['count'] and float(each[0][4 * c + 4]) == ref['count'] / n
    assert bool(((sums - whole).abs() <= 1e-12 * whole.abs()).all())
    val, _ = ops.seg_loss_value(sums, c)
    assert abs(float(val) - ref['loss']) <= ref['value_bound']
    lo = 0
    for sh in parts:
        out = run_seg(sh, None, 1, gamma, alpha, sums=sums)
        hi = lo + sh[0].shape[0]
        S.check(out[3], ref['dlogit'][lo:hi], ref['B_dlogit'][lo:hi], L.K_CE_GRAD, 'shard dlogit')
        S.check(out[4], ref['dyvae'][lo:hi], ref['B_dyvae'][lo:hi], S.K_LOSS_GRAD, 'shard dyvae')
        S.check(out[5], ref['dproj'][lo:hi], ref['B_dproj'][lo:hi], S.K_LOSS_GRAD, 'shard dproj')
        lo = hi


# ---- engine level: the model and crop of the command tests below ---------------------------------------------------------------------
KW = dict(base_filters=16, groups=4, reduction=4, depth=3)
CROP = (16, 16, 16)
N = 2
BF16_LOSS_TOLERANCE = 5e-3          # tests/test_lowp_train_gpu.py: lim['loss'] of bfloat16, between the two engines' first-step losses


@pytest.fixture(scope='module')
def steps():
    """first steps from the same weights, batch, dropout mask and eps: fp32 with DiceVAELoss, with CompoundVAELoss at ce_weight = 0, with
    the focal spec (keeping what the loss was handed), and bfloat16 with the focal spec"""
    import bts_amd  # noqa: F401
    from bts_amd.data import synthetic_batch
    from bts_amd.layers import _base
    from bts_amd.lowp_train import LowPrecisionTrainer
    from bts_amd.model import Model
    from bts_amd.tape import as_tensor, bump_weights_epoch
    from bts_amd.util import CompoundVAELoss, DiceCoefficient, DiceVAELoss, LossSpec, ScheduledOptim, train_step
    _base.set_seed(3)
    m = Model(**KW)
    m.build((N,) + CROP + (2,))
    g = torch.Generator().manual_seed(4)
    for p in m.trainable_variables:
        if p.name.endswith('gamma'):
            p.t.copy_((1.0 + 0.3 * torch.randn(p.t.shape, generator=g)).to(p.t.device))
        elif p.name.endswith('beta') or p.t.dim() == 1:
            p.t.copy_((0.1 * torch.randn(p.t.shape, generator=g)).to(p.t.device))
    bump_weights_epoch()
    x, y, mask, eps = synthetic_batch(N, CROP, latent=KW['base_filters'] * 2 ** (KW['depth'] - 2), seed=99)
    start = m.flat_params.clone()

    class Keeping(CompoundVAELoss):
        def __call__(self, x, y, y_pred, y_vae, z_mean, z_logvar, sample_weight=None):
            fmt = self.data_format
            self.seen = [as_tensor(x, data_format=fmt).t, as_tensor(y, data_format=fmt).t, as_tensor(y_pred, True).t,
                         as_tensor(y_vae, True).t, z_mean.base.t]
            self.seen = [t.detach().contiguous().clone().cpu() for t in self.seen]
            return CompoundVAELoss.__call__(self, x, y, y_pred, y_vae, z_mean, z_logvar, sample_weight)

    def fresh():
        m.flat_params.copy_(start)
        bump_weights_epoch()
        m.encoder.set_dropout_mask(mask)
        m.vae.set_eps(eps)
        opt = ScheduledOptim(1e-4)
        opt(epoch=0)
        return opt

    focal = LossSpec('dice_focal', 1.0, 1.0, 2.0, 0.25)
    out = {'focal': focal}
    out['dice'] = float(train_step(m, fresh(), DiceVAELoss(), DiceCoefficient(), x, y)[0])
    zero = Keeping(spec=LossSpec('dice_ce', 1.0, 0.0))
    out['ce0'] = float(train_step(m, fresh(), zero, DiceCoefficient(), x, y)[0])
    out['ce0_seen'] = zero.seen
    keep = Keeping(spec=focal)
    out['fp32'] = float(train_step(m, fresh(), keep, DiceCoefficient(), x, y)[0])
    out['seen'], out['parts'] = keep.seen, keep.last_parts.cpu()
    tr = LowPrecisionTrainer(m, 'bfloat16', loss=focal)
    out['bf16'] = float(tr.step(fresh(), DiceCoefficient(), x, y)[0])
    torch.cuda.synchronize()
    assert tr.loss_spec == focal
    return out


def test_compound_loss_without_cross_entropy_is_the_dice_loss(steps):
    xs, ys, p, yv, proj = steps['ce0_seen']
    ref = S.loss_ref(p, ys, xs, yv, proj)
    print('DiceVAELoss %.8f, CompoundVAELoss(ce_weight = 0) %.8f, bound %.3e' % (steps['dice'], steps['ce0'], ref['value_bound']))
    assert abs(steps['ce0'] - steps['dice']) <= ref['value_bound']


def test_last_parts_hold_the_cross_entropy_of_the_steps_own_prediction(steps):
    xs, ys, p, yv, proj = steps['seen']
    sp = steps['focal']
    ref = L.seg_loss_ref(p, ys, xs, yv, proj, gamma=sp.gamma, alpha=sp.alpha, w_dice=sp.dice_weight, w_ce=sp.ce_weight)
    parts = steps['parts']
    c = p.shape[-1]
    bound = L.K_CE_SUM * float(ref['B_ce_sums'].sum()) / (ref['count'] * c) + S.EPS32 * ref['ce']
    print('CE %.8f, fp64 %.8f, bound %.3e; dice %.6f l2 %.6f kl %.6f' % (float(parts[3]), ref['ce'], bound, *[float(v) for v in parts[:3]]))
    assert tuple(parts.shape) == (4,) and abs(float(parts[3]) - ref['ce']) <= bound
    assert abs(float(parts[0]) - ref['dice']) <= 4 * S.EPS32 and ref['ce'] > 0
    assert steps['fp32'] > steps['dice']                 # the focal term is positive and is in the step's loss


def test_bfloat16_trainer_with_the_spec_agrees_with_the_fp32_step(steps):
    dl = abs(steps['bf16'] - steps['fp32']) / abs(steps['fp32'])
    print('first-step loss: bfloat16 %.6f, float32 %.6f (rel %.2e); Dice loss alone %.6f' % (steps['bf16'], steps['fp32'], dl, steps['dice']))
    assert dl <= BF16_LOSS_TOLERANCE
    assert abs(steps['bf16'] - steps['dice']) / steps['dice'] > BF16_LOSS_TOLERANCE      # (the spec reached the 16-bit engine)


# ---- the command -------------------------------------------------------------------------------------------------------------------------
SIZE = (20, 18, 22, 2)
MODEL_FLAGS = ['--crop_size', '16,16,16', '--base_filters', '16', '--groups', '4', '--reduction', '4', '--depth', '3', '--batch_size', '2']
NAMES = ('train_loss', 'train_macro_dice', 'train_micro_dice', 'val_loss', 'val_macro_dice', 'val_micro_dice')
FOCAL_FLAGS = ['--targets', 'regions', '--out_ch', '3', '--loss', 'dice_focal', '--focal_alpha', '0.25']
FOCAL_STORED = dict(loss='dice_focal', dice_weight=1.0, ce_weight=1.0, focal_gamma=2.0, focal_alpha=0.25)


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    """the dataset of tests/test_train_cli_gpu.py: 5 training and 2 validation examples of 20x18x22x2 with labels 0..3"""
    loc = str(tmp_path_factory.mktemp('loss_dataset'))
    rs = np.random.RandomState(5)
    for sub, n in (('train', 5), ('val', 2)):
        os.makedirs(os.path.join(loc, sub))
        for i in range(n):
            lab = (rs.rand(*SIZE[:3]) * 4).astype(np.int64).astype(np.float32)[..., None]
            np.savez(os.path.join(loc, sub, 'ex%d.npz' % i), x=rs.randn(*SIZE).astype(np.float32), y=lab)
    np.save(os.path.join(loc, 'prepro.npy'), {'size': dict(zip('hwdc', SIZE)), 'norm': {'mean': np.zeros(2), 'std': np.ones(2)}},
            allow_pickle=True)
    return loc


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


def test_train_command_with_the_focal_loss_in_float32_and_a_resumed_run(folder, tmp_path, capsys):
    from bts_amd.util import CompoundVAELoss, LossSpec
    out = os.path.join(str(tmp_path), 'run')
    T, res = _train(_argv(folder, out, '--n_epochs', '2', '--data_format', 'channels_last', '--patience', '5', *FOCAL_FLAGS))
    assert 'Loss: 1 * Dice + 1 * focal (gamma 2, alpha 0.25)' in capsys.readouterr().out
    _log_is_finite(T, out, 2)
    stored = T.load_train_args(out)
    assert {k: stored[k] for k in T.LOSS_KEYS} == FOCAL_STORED and len(res['history']) == 2
    _, meta = T.read_container(os.path.join(out, T.CHECKPOINT_NAME))
    argv = ['--train_loc', os.path.join(folder, 'train'), '--val_loc', os.path.join(folder, 'val'), '--prepro_loc',
            os.path.join(folder, 'prepro.npy'), '--load_folder', out, '--batch_size', '2', '--n_epochs', '3', '--patience', '5',
            '--loss', 'dice']
    args = T.parse_args(argv)
    assert args.loss == 'dice_focal' and args.focal_alpha == 0.25
    seen = []
    real = T.fit

    def spy(model, optimizer, loss_fn, *a, **k):
        seen.append((type(loss_fn), loss_fn.spec))
        return real(model, optimizer, loss_fn, *a, **k)
    T.fit = spy
    try:
        res2 = T.run(args)
    finally:
        T.fit = real
    assert seen == [(CompoundVAELoss, LossSpec('dice_focal', 1.0, 1.0, 2.0, 0.25))]
    assert [h['epoch'] for h in res2['history']] == list(range(meta['next_epoch'], 3)) and len(res2['history']) >= 1
    assert all(np.isfinite([float(h[k]) for k in NAMES]).all() for h in res2['history'])
    assert {k: T.load_train_args(out)[k] for k in T.LOSS_KEYS} == FOCAL_STORED


def test_train_command_with_the_focal_loss_in_bfloat16(folder, tmp_path):
    from bts_amd.util import LossSpec
    out = os.path.join(str(tmp_path), 'run16')
    T, res = _train(_argv(folder, out, '--n_epochs', '2', '--data_format', 'channels_first', '--dtype', 'bfloat16', *FOCAL_FLAGS))
    _log_is_finite(T, out, 2)
    stored = T.load_train_args(out)
    assert {k: stored[k] for k in T.LOSS_KEYS} == FOCAL_STORED
    assert res['model']._trainer16.loss_spec == LossSpec('dice_focal', 1.0, 1.0, 2.0, 0.25)
    assert os.path.exists(os.path.join(out, T.CHECKPOINT_NAME))
    # a resumed run keeps the loss and continues at the recorded epoch
    _, meta = T.read_container(os.path.join(out, T.CHECKPOINT_NAME))
    args = T.parse_args(['--train_loc', os.path.join(folder, 'train'), '--val_loc', os.path.join(folder, 'val'), '--prepro_loc',
                         os.path.join(folder, 'prepro.npy'), '--load_folder', out, '--batch_size', '2', '--n_epochs', '3',
                         '--dtype', 'bfloat16'])
    assert args.loss == 'dice_focal'
    res2 = T.run(args)
    assert res2['model']._trainer16.loss_spec == LossSpec('dice_focal', 1.0, 1.0, 2.0, 0.25)
    assert [h['epoch'] for h in res2['history']] == list(range(meta['next_epoch'], 3))
    assert all(np.isfinite([float(h[k]) for k in NAMES]).all() for h in res2['history'])


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_spelling_the_default_loss_changes_nothing(folder, tmp_path, dtype):
    logs = []
    for name, more in (('plain', []), ('spelled', ['--loss', 'dice'])):
        out = os.path.join(str(tmp_path), name)
        T, res = _train(_argv(folder, out, '--n_epochs', '2', '--data_format', 'channels_last', '--dtype', dtype, *more))
        logs.append(open(os.path.join(out, 'train.log'), 'rb').read())
        assert T.load_train_args(out)['loss'] == 'dice'
        if dtype != 'float32':
            assert res['model']._trainer16.loss_spec is None
    assert logs[0] == logs[1] and logs[0].count(b'\n') == 3
