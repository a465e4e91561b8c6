"""No GPU: the compound loss (csrc/loss_ce.hip, util.LossSpec, the --loss flags).  The fp32 restatement of tests/loss_ce_ref.py sits
within K/4 of its bounds; the fp64 reference is torch's binary cross-entropy at gamma = 0 and agrees with finite differences, the
clamp edges included; the C ABI refuses bad arguments before any HIP call; the command's flags, refusals and train_args.pkl."""
import math
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import loss_ce_ref as L  # noqa: E402

F64 = torch.float64


# ---- restatement against reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gamma,alpha', L.CASES)
@pytest.mark.parametrize('shape', L.LOSS_SHAPES_SMALL)
def test_restatement_within_a_quarter_of_the_bounds(shape, gamma, alpha):
    n, dims, c, cx, lz = shape
    host = L.loss_inputs(n, dims, c, cx, lz)
    sums = L.seg_sums_f32(*host, gamma=gamma, alpha=alpha)
    first = True
    for ts in (1, 0):
        for gs in (1.0, 0.125, 65536.0):
            ref = L.seg_loss_ref(*host, gs=gs, through_sigmoid=ts, gamma=gamma, alpha=alpha, w_dice=0.75, w_ce=1.5)
            if first:
                L.check(sums[3 * c + 4:4 * c + 4], ref['ce_sums'], ref['B_ce_sums'], L.K_CE_SUM / 4, 'restated CE sums')
                assert float(sums[4 * c + 4]) == ref['count'] == n * dims[0] * dims[1] * dims[2]
                val, parts = L.seg_value_f64(sums, c, True, 0.75, 1.5)
                print('value: err %.3e, bound %.3e' % (abs(val - ref['loss']), ref['value_bound']))
                assert abs(val - ref['loss']) <= ref['value_bound']
                assert abs(parts[3] - ref['ce']) <= L.K_CE_SUM / 4 * float(ref['B_ce_sums'].sum()) / (ref['count'] * c) + L.EPS32 * ref['ce']
                first = False
            dl, dyv, dpr = L.seg_bwd_f32(*host, sums, gs=gs, through_sigmoid=ts, gamma=gamma, alpha=alpha, w_dice=0.75, w_ce=1.5)
            L.check(dl, ref['dlogit'], ref['B_dlogit'], L.K_CE_GRAD / 4, 'restated dlogit ts=%d gs=%g' % (ts, gs))


def test_restatement_at_the_clamp_and_on_soft_targets():
    p, t = L.saturation_inputs()
    for gamma, alpha in L.CASES:
        for ts in (1, 0):
            ref = L.seg_loss_ref(p, t, through_sigmoid=ts, gamma=gamma, alpha=alpha)
            sums = L.seg_sums_f32(p, t, None, None, None, gamma=gamma, alpha=alpha)
            assert bool(torch.isfinite(sums).all())
            L.check(sums[13:16], ref['ce_sums'], ref['B_ce_sums'], L.K_CE_SUM / 4, 'saturated CE sums')
            dl, _, _ = L.seg_bwd_f32(p, t, None, None, None, sums, through_sigmoid=ts, gamma=gamma, alpha=alpha)
            assert bool(torch.isfinite(dl).all())
            L.check(dl, ref['dlogit'], ref['B_dlogit'], L.K_CE_GRAD / 4, 'saturated dlogit')
            outside = (p < L.EPS) | (p > 1.0 - L.EPS)
            assert bool((ref['dlogit_ce'][outside] == 0).all()) and int(outside.sum()) == p.numel() * 4 // 6
            on_edge = (p.double() == L.EPS) | (p.double() == 1.0 - L.EPS)
            assert bool((ref['dlogit_ce'][on_edge & (((t == 1) & (p < 0.5)) | ((t == 0) & (p > 0.5)))] != 0).all())
    n, dims, c, cx, lz = L.LOSS_SHAPES_SMALL[0]
    host = list(L.loss_inputs(n, dims, c, cx, lz))
    host[1] = L.soft_targets(host[1].shape)
    assert set(host[1].unique().tolist()) == {0.0, 0.25, 1.0}
    ref = L.seg_loss_ref(*host, gamma=2.0, alpha=0.25)
    sums = L.seg_sums_f32(*host, gamma=2.0, alpha=0.25)
    L.check(sums[3 * c + 4:4 * c + 4], ref['ce_sums'], ref['B_ce_sums'], L.K_CE_SUM / 4, 'soft-target CE sums')
    dl, _, _ = L.seg_bwd_f32(*host, sums, gamma=2.0, alpha=0.25)
    L.check(dl, ref['dlogit'], ref['B_dlogit'], L.K_CE_GRAD / 4, 'soft-target dlogit')


# ---- the reference itself --------------------------------------------------------------------------------------------------------------
def test_reference_at_gamma_zero_is_binary_cross_entropy():
    n, dims, c, cx, lz = L.LOSS_SHAPES_SMALL[0]
    p, y = L.loss_inputs(n, dims, c, cx, lz)[:2]
    ref = L.seg_loss_ref(p, y, gamma=0.0)
    q = torch.clamp(p.double(), L.EPS, 1.0 - L.EPS)
    want = float(torch.nn.functional.binary_cross_entropy(q, y.double()))
    assert abs(ref['ce'] - want) <= 1e-12 * want
    # the two bounds of the clamp are fp32 numbers, and Keras' 1 - 1e-7 rounds to the upper one
    assert float(np.float32(L.EPS)) == L.EPS and float(np.float32(1.0 - L.EPS)) == 1.0 - L.EPS
    assert float(np.float32(1.0 - 1e-7)) == 1.0 - L.EPS


@pytest.mark.parametrize('gamma,alpha', L.CASES)
def test_reference_gradient_against_finite_differences(gamma, alpha):
    """central differences in float64 at interior elements; ON a clamp edge the function has a kink: the one-sided difference into the
    interval is the gradient torch.clamp's autograd gives, the one out of it is zero, so the central difference is half the gradient"""
    g, wp, wn = L.weights(gamma, alpha)
    p = torch.tensor([0.3, 0.9, 1e-3, 0.5, 1.0 - 1e-4, L.EPS, 1.0 - L.EPS, L.EPS, 1.0 - L.EPS], dtype=F64)
    t = torch.tensor([1.0, 0.0, 0.0, 0.25, 1.0, 1.0, 0.0, 0.0, 1.0], dtype=F64)
    pd = p.clone().requires_grad_(True)
    L.ce_value64(pd, t, g, wp, wn).backward()
    grad = pd.grad

    def diff(i, lo, hi):      # of element i's own term (the other elements' terms do not change: their rounding is kept out of the quotient)
        a, b = p[i:i + 1] + lo, p[i:i + 1] + hi
        return float(L.ce_terms64(b, t[i:i + 1], g, wp, wn) - L.ce_terms64(a, t[i:i + 1], g, wp, wn)) / (hi - lo) / p.numel()
    for i in range(5):
        h = 1e-4 * min(float(p[i]), 1.0 - float(p[i]))
        fd = diff(i, -h, h)
        assert abs(fd - float(grad[i])) <= 1e-6 * abs(float(grad[i])) + 1e-12, (i, fd, float(grad[i]))
    for i in range(5, 9):
        h = 1e-4 * L.EPS
        inward = 1.0 if float(p[i]) < 0.5 else -1.0
        fd_in, fd_out, fd_c = diff(i, 0.0, inward * h) , diff(i, 0.0, -inward * h), diff(i, -h, h)
        assert fd_out == 0.0
        assert abs(fd_in - float(grad[i])) <= 1e-3 * abs(float(grad[i])) + 1e-12, (i, fd_in, float(grad[i]))
        assert abs(fd_c - 0.5 * float(grad[i])) <= 1e-3 * abs(float(grad[i])) + 1e-12
    assert float(grad[5]) < 0 and float(grad[6]) > 0           # the loss pulls a saturated wrong answer back


def test_through_sigmoid_form_needs_no_division():
    """the forms of the issue: d e / d q * q (1 - q) = w_pos t [gamma q (1-q)^gamma log q - (1-q)^(gamma+1)] + w_neg (1-t) [...]"""
    p = torch.linspace(0.01, 0.99, 37, dtype=F64)
    for t in (0.0, 0.25, 1.0):
        for gamma, alpha in L.CASES:
            g, wp, wn = L.weights(gamma, alpha)
            pd = p.clone().requires_grad_(True)
            L.ce_terms64(pd, torch.full_like(p, t), g, wp, wn).sum().backward()
            pos = g * p * (1 - p) ** g * torch.log(p) - (1 - p) ** (g + 1)
            neg = -g * p ** g * (1 - p) * torch.log(1 - p) + p ** (g + 1)
            want = wp * t * pos + wn * (1 - t) * neg
            assert float((pd.grad * p * (1 - p) - want).abs().max()) <= 1e-13
            if g == 0.0 and alpha is None:
                assert float((want - (p - t)).abs().max()) <= 1e-15


# ---- the C ABI refuses bad arguments before any HIP call -----------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib, parse_header
    lb = lib()
    protos = parse_header()
    for name in ('bts_seg_loss_workspace', 'bts_seg_loss_sums', 'bts_seg_loss_value', 'bts_seg_loss_bwd'):
        assert name in protos
    assert [a for _, a in protos['bts_seg_loss_sums'][1]][:17] == [a for _, a in protos['bts_loss_sums'][1]][:17]
    assert [a for _, a in protos['bts_seg_loss_sums'][1]][17:] == ['gamma', 'w_pos', 'w_neg', 'stream']
    assert [a for _, a in protos['bts_seg_loss_bwd'][1]][:20] == [a for _, a in protos['bts_loss_bwd'][1]][:20]
    assert [a for _, a in protos['bts_seg_loss_bwd'][1]][20:] == ['w_dice', 'w_ce', 'gamma', 'w_pos', 'w_neg', 'stream']
    SHAPE, UNSUPPORTED, WORKSPACE = -1, -3, -4
    nb = lb._bts_seg_loss_workspace()
    assert nb >= 1024 * 33 * 8 and nb > lb._bts_loss_workspace()
    inf, nan = float('inf'), float('nan')

    def sums(N=2, V=64, C=3, ldp=3, ldy=3, gamma=2.0, w_pos=1.0, w_neg=1.0, ws=nb):
        return lb._bts_seg_loss_sums(None, None, None, None, None, None, None, ws, N, V, C, ldp, ldy, 0, 0, 0, 0, gamma, w_pos, w_neg, None)

    def bwd(N=2, V=64, C=3, ldp=3, ldy=3, w_dice=1.0, w_ce=1.0, gamma=2.0, w_pos=1.0, w_neg=1.0):
        return lb._bts_seg_loss_bwd(None, None, None, None, None, None, None, None, None, None, N, V, C, ldp, ldy, 0, 0, 0, 0, 1,
                                    w_dice, w_ce, gamma, w_pos, w_neg, None)
    for call in (sums, bwd):
        assert call(C=0) == SHAPE and call(C=9, ldp=9, ldy=9) == SHAPE
        assert call(N=0) == SHAPE and call(N=-1) == SHAPE and call(V=0) == SHAPE
        assert call(ldp=2) == SHAPE and call(ldy=2) == SHAPE
        for bad in (-0.5, 8.5, inf, nan):
            assert call(gamma=bad) == UNSUPPORTED, bad
        for bad in (-1.0, inf, nan):
            assert call(w_pos=bad) == UNSUPPORTED and call(w_neg=bad) == UNSUPPORTED, bad
    for bad in (-1.0, inf, nan):
        assert bwd(w_dice=bad) == UNSUPPORTED and bwd(w_ce=bad) == UNSUPPORTED
        assert lb._bts_seg_loss_value(None, None, None, 3, 1, bad, 1.0, None) == UNSUPPORTED
        assert lb._bts_seg_loss_value(None, None, None, 3, 1, 1.0, bad, None) == UNSUPPORTED
    assert lb._bts_seg_loss_value(None, None, None, 0, 1, 1.0, 1.0, None) == SHAPE
    assert lb._bts_seg_loss_value(None, None, None, 9, 1, 1.0, 1.0, None) == SHAPE
    assert sums(ws=nb - 1) == WORKSPACE and sums(ws=0) == WORKSPACE
    # with VAE operands (a non-null x; never dereferenced by a refused call): their voxel strides are checked too
    import ctypes
    x = ctypes.c_void_p(64)
    assert lb._bts_seg_loss_sums(None, None, x, x, None, None, None, nb, 2, 64, 3, 3, 3, 2, 1, 2, 4, 0.0, 1.0, 1.0, None) == SHAPE
    assert lb._bts_seg_loss_sums(None, None, x, x, None, None, None, nb, 2, 64, 3, 3, 3, 2, 2, 1, 4, 0.0, 1.0, 1.0, None) == SHAPE


# ---- LossSpec ----------------------------------------------------------------------------------------------------------------------------
def test_loss_spec_is_a_validated_value_object():
    import bts_amd  # noqa: F401
    from bts_amd.util import CompoundVAELoss, DiceVAELoss, LossSpec
    s = LossSpec('dice_focal', 0.5, 2, 2.0, 0.25)
    assert (s.kind, s.dice_weight, s.ce_weight, s.gamma, s.alpha) == ('dice_focal', 0.5, 2.0, 2.0, 0.25)
    assert s == LossSpec('dice_focal', 0.5, 2.0, 2, 0.25) and hash(s) == hash(LossSpec('dice_focal', 0.5, 2.0, 2, 0.25))
    assert s != LossSpec('dice_focal', 0.5, 2.0, 2.0, None) and s != LossSpec('dice_ce', 0.5, 2.0, 2.0, 0.25)
    assert s.kernel_args == (2.0, 0.25, 0.75) and LossSpec('dice_focal', gamma=0.5).kernel_args == (0.5, 1.0, 1.0)
    assert LossSpec('dice_ce', gamma=3.0, alpha=0.3).kernel_args == (0.0, 1.0, 1.0)              # dice_ce ignores the focal fields
    assert LossSpec() == LossSpec('dice_ce', 1.0, 1.0, 2.0, None)
    with pytest.raises(AttributeError):
        s.gamma = 1.0
    for kw, word in ((dict(kind='dice'), 'kind'), (dict(kind='focal'), 'kind'), (dict(dice_weight=-1), 'dice_weight'),
                     (dict(ce_weight=float('nan')), 'ce_weight'), (dict(ce_weight=float('inf')), 'ce_weight'),
                     (dict(kind='dice_focal', gamma=-0.1), 'gamma'), (dict(kind='dice_focal', gamma=8.5), 'gamma'),
                     (dict(kind='dice_focal', gamma=float('nan')), 'gamma'), (dict(kind='dice_focal', alpha=0.0), 'alpha'),
                     (dict(kind='dice_focal', alpha=1.0), 'alpha')):
        with pytest.raises(ValueError, match=word):
            LossSpec(**kw)
    fn = CompoundVAELoss(data_format='channels_first', spec=s)
    assert fn.spec is s and fn.data_format == 'channels_first' and fn.last_parts is None
    assert CompoundVAELoss().spec == LossSpec() and not hasattr(DiceVAELoss(), 'spec')
    with pytest.raises(ValueError):
        CompoundVAELoss(data_format='NCDHW')
    with pytest.raises(TypeError):
        CompoundVAELoss(spec='dice_ce')


# ---- the command -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def prepro(tmp_path):
    path = os.path.join(str(tmp_path), 'prepro.npy')
    np.save(path, {'size': {'h': 20, 'w': 18, 'd': 22, 'c': 3}, 'norm': {'mean': np.zeros(3), 'std': np.ones(3)}}, allow_pickle=True)
    return path


def _argv(prepro, *more):
    return ['--train_loc', 'tr', '--val_loc', 'va', '--prepro_loc', prepro] + list(more)


def _T():
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    return T


def test_flags_defaults_and_where_they_live(prepro):
    T = _T()
    from bts_amd.util import LossSpec
    act = {a.option_strings[0]: a for a in T.full_parser()._actions if a.option_strings}
    assert act['--loss'].default == 'dice' and list(act['--loss'].choices) == ['dice', 'dice_ce', 'dice_focal']
    assert act['--dice_weight'].default == 1.0 and act['--ce_weight'].default == 1.0 and act['--focal_gamma'].default == 2.0
    assert act['--focal_alpha'].default is None
    # arg_parser() keeps its pinned flag set: the reference's 21 flags and the four of tests/test_train_cli_host.py
    base = {a.option_strings[0] for a in T.arg_parser()._actions if a.option_strings and a.dest != 'help'}
    assert len(base) == 25 and not base & {'--loss', '--dice_weight', '--ce_weight', '--focal_gamma', '--focal_alpha'}
    args = T.parse_args(_argv(prepro))
    assert (args.loss, args.dice_weight, args.ce_weight, args.focal_gamma, args.focal_alpha) == ('dice', 1.0, 1.0, 2.0, None)
    assert T.loss_spec(args) is None
    args = T.parse_args(_argv(prepro, '--loss', 'dice_focal', '--focal_alpha', '0.25', '--ce_weight', '0.5'))
    assert T.loss_spec(args) == LossSpec('dice_focal', 1.0, 0.5, 2.0, 0.25)
    # dice_ce ignores the focal flags
    args = T.parse_args(_argv(prepro, '--loss', 'dice_ce', '--focal_gamma', '99', '--focal_alpha', '7', '--dice_weight', '2'))
    assert T.loss_spec(args).kernel_args == (0.0, 1.0, 1.0) and T.loss_spec(args).dice_weight == 2.0
    # the focal flags are of no consequence with the default loss either
    assert T.loss_spec(T.parse_args(_argv(prepro, '--focal_gamma', '1.5'))) is None


@pytest.mark.parametrize('more,word', [(['--loss', 'dice', '--dice_weight', '0.5'], '--dice_weight'),
                                       (['--ce_weight', '2'], '--ce_weight'),
                                       (['--loss', 'dice_ce', '--dice_weight', '-1'], '--dice_weight'),
                                       (['--loss', 'dice_focal', '--ce_weight', 'nan'], '--ce_weight'),
                                       (['--loss', 'dice_focal', '--focal_gamma', '-1'], '--focal_gamma'),
                                       (['--loss', 'dice_focal', '--focal_gamma', '9'], '--focal_gamma'),
                                       (['--loss', 'dice_focal', '--focal_alpha', '0'], '--focal_alpha'),
                                       (['--loss', 'dice_focal', '--focal_alpha', '1'], '--focal_alpha')])
def test_refusals_by_name_at_parse_time(prepro, tmp_path, more, word):
    T = _T()
    out = os.path.join(str(tmp_path), 'run')
    with pytest.raises(ValueError, match=word):
        T.parse_args(_argv(prepro, '--save_folder', out, *more))
    assert not os.path.exists(os.path.join(out, T.ARGS_NAME))          # refused before anything is written
    with pytest.raises(SystemExit):
        T.parse_args(_argv(prepro, '--loss', 'focal'))


def test_train_args_round_trip_and_an_older_pickle(prepro, tmp_path):
    T = _T()
    from bts_amd.util import LossSpec
    out = os.path.join(str(tmp_path), 'run')
    model = ['--crop_size', '16,16,16', '--base_filters', '16', '--groups', '4', '--reduction', '4', '--depth', '3']
    T.parse_args(_argv(prepro, '--save_folder', out, '--loss', 'dice_focal', '--focal_alpha', '0.25', '--focal_gamma', '1.5',
                       '--dice_weight', '0.5', *model))
    stored = T.load_train_args(out)
    assert {k: stored[k] for k in T.LOSS_KEYS} == dict(loss='dice_focal', dice_weight=0.5, ce_weight=1.0, focal_gamma=1.5, focal_alpha=0.25)
    # --load_folder restores them, whatever the command line says
    again = T.parse_args(_argv(prepro, '--load_folder', out, '--loss', 'dice_ce', '--ce_weight', '3'))
    assert T.loss_spec(again) == LossSpec('dice_focal', 0.5, 1.0, 1.5, 0.25)
    assert {k: T.load_train_args(out)[k] for k in T.LOSS_KEYS} == {k: stored[k] for k in T.LOSS_KEYS}
    # a pickle from before the flags existed means `dice`, and flags on the command line do not change that
    old = dict(stored)
    for k in T.LOSS_KEYS:
        del old[k]
    older = os.path.join(str(tmp_path), 'older')
    os.makedirs(older)
    with open(os.path.join(older, T.ARGS_NAME), 'wb') as f:
        pickle.dump(old, f)
    args = T.parse_args(_argv(prepro, '--load_folder', older, '--loss', 'dice_focal', '--ce_weight', '3'))
    assert args.loss == 'dice' and T.loss_spec(args) is None and math.isclose(args.ce_weight, 1.0)
    assert T.load_train_args(older)['loss'] == 'dice'
