"""CPU: the tolerances tests/test_step_kernels_gpu.py applies are honest, the generator restatement it compares bit for bit has
the statistics a generator needs, and the step kernels' entry points turn bad arguments away before any HIP call.

Every fp32 restatement of tests/step_ref.py (the cited formula in torch float32, in the documented order) must stay within K/4 of
the bound its kernel is held to with K -- or within the bound itself / the rounding count where step_ref's docstring says why.
Each test prints the ratio it measured (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import step_ref as S  # noqa: E402


def held(what, got, ref, unit, limit):
    r = S.ratio(got, ref, unit)
    print('%-46s %.3f (limit %g)' % (what, r, limit))
    assert r <= limit, '%s: the fp32 restatement is %.3f x eps32*B from the reference, limit %g' % (what, r, limit)
    return r


# ---------------------------------------------------------------------------------------------------------------
# restatement against reference
# ---------------------------------------------------------------------------------------------------------------
def _loss_case(shape, gs, ts, vae=True):
    n, dims, c, cx, lz = shape
    p, y, x, yv, proj = S.loss_inputs(n, dims, c, cx, lz)
    if not vae:
        x = yv = proj = None
    ref = S.loss_ref(p, y, x, yv, proj, gs, ts)
    sums = S.loss_sums_f32(p, y, x, yv, proj)
    for k, name in enumerate('IPT'):
        held('loss sums %s %s' % (name, (shape,)), sums[k * c:(k + 1) * c], ref[name], S.EPS32 * ref[name], 1.0)
    val, parts = S.loss_value_f64(sums, c, vae)
    assert abs(val - ref['loss']) <= ref['value_bound'] / 4, (val, ref['loss'], ref['value_bound'])
    g, dyv, dproj = S.loss_bwd_f32(p, y, x, yv, proj, sums, gs, ts)
    lim = S.K_LOSS_GRAD / 4
    out = [held('dlogit %s gs=%g ts=%d' % (shape, gs, ts), g, ref['dlogit'], ref['B_dlogit'], lim)]
    if vae:
        out.append(held('dyvae', dyv, ref['dyvae'], ref['B_dyvae'], lim))
        out.append(held('dproj mean', dproj[:, :lz], ref['dproj'][:, :lz], ref['B_dproj'][:, :lz], lim))
        out.append(held('dproj logvar', dproj[:, lz:], ref['dproj'][:, lz:], ref['B_dproj'][:, lz:], lim))
        assert abs(sums[3 * c] - ref['sq']) <= 4 * S.EPS32 * ref['sq']
        assert abs(sums[3 * c + 1] - ref['klsum']) <= 4 * S.EPS32 * ref['klabs']
        assert float(sums[3 * c + 2]) == ref['numel_x'] and float(sums[3 * c + 3]) == ref['numel_z']
    else:
        assert parts[1] == 0.0 and parts[2] == 0.0 and abs(val - ref['dice']) <= 4 * S.EPS32
    return out


@pytest.mark.parametrize('shape', S.LOSS_SHAPES_SMALL)
@pytest.mark.parametrize('ts', [0, 1])
@pytest.mark.parametrize('gs', [1.0, 0.125, 65536.0])
def test_loss_restatement_small(shape, ts, gs):
    _loss_case(shape, gs, ts)
    _loss_case(shape, gs, ts, vae=False)


@pytest.mark.parametrize('shape', [S.LOSS_SHAPE_PAST_PARTIAL, S.LOSS_SHAPE_PAST_BWD])
def test_loss_restatement_large(shape):
    _loss_case(shape, 1.0, 1)


@pytest.mark.parametrize('gmul', [1.0, 0.125, 1.0 / 65536])
@pytest.mark.parametrize('p0_zero', [True, False])
def test_adam_restatement(gmul, p0_zero):
    n = 10007
    g1 = S.adam_grad(n, 1, gmul)
    p = torch.zeros(n) if p0_zero else torch.randn(n, generator=torch.Generator().manual_seed(5))
    m, v = torch.zeros(n), torch.zeros(n)
    for t, g in ((1, g1), (2, g1 * -0.7), (3, g1)):
        sc = S.adam_scalars(t)
        (pr, mr, vr), (Bp, Bm, Bv) = S.adam_ref(p, g, m, v, *sc, gmul)
        p2, m2, v2 = S.adam_f32(p, g, m, v, *sc, gmul)
        for what, a, b, B in (('p', p2, pr, Bp), ('m', m2, mr, Bm), ('v', v2, vr, Bv)):
            held('adam %s step %d gmul %g' % (what, t, gmul), a, b, B, S.K_ADAM / 4)
        p, m, v = p2, m2, v2


def test_adam_bound_pins_the_place_of_epsilon():
    """sqrt(v + eps) in place of sqrt(v) + eps differs only where sqrt(v) is not >> eps: at |g| ~ 1e-8 and below.  From p0 = 0
    the bound on p is K eps32 times the update itself, so the wrong form is thousands of bounds away."""
    n = 10007
    g = S.adam_grad(n, 1, 1.0)
    z = torch.zeros(n)
    sc = S.adam_scalars(1)
    (pr, _, _), (Bp, _, _) = S.adam_ref(z, g, z, z, *sc, 1.0)
    wrong, _, _ = S.adam_f32(z, g, z, z, *sc, 1.0, eps_inside=True)
    assert S.ratio(wrong, pr, Bp) > 1000 * S.K_ADAM
    one = torch.tensor([1e-8])
    (pr1, _, _), _ = S.adam_ref(z[:1], one, z[:1], z[:1], *sc, 1.0)
    w1, _, _ = S.adam_f32(z[:1], one, z[:1], z[:1], *sc, 1.0, eps_inside=True)
    print('update at g = 1e-8, step 1: eps outside %.3e, eps inside %.3e (in units of lr)' % (float(pr1) / 1e-4, float(w1) / 1e-4))


@pytest.mark.parametrize('shape', S.DENSE_SHAPES)
def test_dense_restatement(shape):
    n, fin, fout, relu = shape
    x, w, b, dy = S.dense_inputs(n, fin, fout)
    for bias in (b, None):
        ref, B = S.dense_fwd_ref(x, w, bias, relu)
        held('dense fwd %s bias=%s' % (shape, bias is not None), S.dense_fwd_f32(x, w, bias, relu), ref, B, S.K_DENSE / 4)
    (dxr, dwr, dbr), (Bx, Bw, Bb) = S.dense_bwd_ref(x, w, dy)
    dx, dw, db = S.dense_bwd_f32(x, w, dy)
    held('dense dx', dx, dxr, Bx, S.K_DENSE / 4)
    held('dense dw (chain of %d)' % n, dw, dwr, Bw, S.dense_short_chain_limit(n))
    held('dense db (chain of %d)' % n, db, dbr, Bb, S.dense_short_chain_limit(n))


def test_l2_restatement():
    g0 = torch.Generator().manual_seed(9)
    p, g = torch.randn(700000, generator=g0), torch.randn(700000, generator=g0)
    for ranges in ([(3, 1, 1e-5)], [(0, 4000, 1e-5), (4000, 3001, 3e-5)], [(17, 600001, 2e-5)]):
        for gs in (1.0, 65536.0):
            val, vb, gr, B = S.l2_ref(p, g, ranges, gs)
            v32, g32 = S.l2_f32(p, g, ranges, gs)
            assert abs(v32 - val) <= vb, (v32, val, vb)
            held('l2 grad %d ranges gs=%g' % (len(ranges), gs), g32, gr, B, S.K_L2_GRAD / 4)


def test_colsum_and_moments_restatement():
    g0 = torch.Generator().manual_seed(10)
    x = torch.randn((3, 1000, 20), generator=g0)
    old = torch.randn((3, 20), generator=g0)
    for scale in (1.0, 1.0 / 1000):
        for son in (False, True):
            o = old[0] if son else old
            for acc in (None, o):
                ref, bound = S.colsum_ref(x, scale, son, acc)
                held('colsum scale=%g sum_over_n=%d acc=%d' % (scale, son, acc is not None), S.colsum_f32(x, scale, son, acc), ref,
                     bound, 1.0)
    v = torch.randn((48 * 48 * 64, 2), generator=g0) + 1000.0
    mr, vr, mb, vb = S.moments_ref(v)
    m32, v32 = S.moments_f32(v)
    held('moments mean (mean 1000, sd 1)', m32, mr, mb, 1.0)
    held('moments var  (mean 1000, sd 1)', v32, vr, vb, 1.0)
    c = torch.full((4096, 3), 1000.1)
    assert torch.equal(S.moments_f32(c)[1], torch.zeros(3))


def test_elementwise_restatement():
    g0 = torch.Generator().manual_seed(11)
    x, y = torch.randn(100000, generator=g0), torch.randn(100000, generator=g0)
    ref, B = S.axpy_ref(y, x, -0.37)
    held('axpy', S.axpy_f32(y, x, -0.37), ref, B, S.K_EW / 4)
    s = torch.sigmoid(x * 3)
    ref, B = S.sigmoid_bwd_ref(s, y)
    held('sigmoid_bwd (3 roundings)', S.sigmoid_bwd_f32(s, y), ref, B, S.ROUNDINGS['sigmoid_bwd'])
    mask = torch.from_numpy(S.dropout_mask_np(100000, 0.2, 1234))
    ref, B = S.dropout_apply_ref(x, mask, 0.2)
    held('dropout_apply (3 roundings)', S.dropout_apply_f32(x, mask, 0.2), ref, B, S.ROUNDINGS['dropout_apply'])
    assert torch.equal(S.dropout_apply_f32(x, torch.ones_like(mask), 0.0), x)
    a, b = x[:1], y[:1]
    for bb in (None, b):
        ref, B = S.lincomb_ref(a, bb, 1.0, 0.3)
        held('scalar_lincomb b=%s' % (bb is not None), S.lincomb_f32(a, bb, 1.0, 0.3), ref, B, S.K_EW / 4)
    for n, lz in ((1, 1), (3, 8), (5, 128)):
        proj, eps, dz, old = [torch.randn(sh, generator=g0) for sh in ((n, 2 * lz), (n, lz), (n, lz), (n, 2 * lz))]
        zr, Bz, dr, Bd = S.vae_sample_ref(proj, eps, dz, old)
        z, d = S.vae_sample_f32(proj, eps, dz, old)
        held('vae sample fwd (%d,%d)' % (n, lz), z, zr, Bz, S.ROUNDINGS['vae_sample'])
        held('vae sample bwd (%d,%d)' % (n, lz), d, dr, Bd, S.ROUNDINGS['vae_sample'])


def test_normal_restatement():
    for seed in (7, 1234):
        ref, unit = S.normal_ref(1 << 16, seed)
        x = S.normal_f32(1 << 16, seed)
        held('normal seed %d' % seed, torch.from_numpy(x.astype(np.float64)), torch.from_numpy(ref), torch.from_numpy(unit),
             S.ROUNDINGS['normal'])
        assert np.abs(x).max() <= S.NORMAL_MAX


# ---------------------------------------------------------------------------------------------------------------
# statistics of the generator (numpy restatement; the GPU test holds the kernels to it bit for bit)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [7, 1234])
def test_generator_statistics(seed):
    n = 1 << 20
    x = S.normal_f32(n, seed).astype(np.float64)
    x2 = S.normal_f32(n, seed + 1).astype(np.float64)
    stats = [('mean', x.mean(), 1 / np.sqrt(n)), ('variance - 1', (x * x).mean() - 1, np.sqrt(2 / n)),
             ('third moment', (x ** 3).mean(), np.sqrt(15 / n)), ('fourth moment - 3', (x ** 4).mean() - 3, np.sqrt(96 / n)),
             ('lag-1 product', (x[:-1] * x[1:]).mean(), 1 / np.sqrt(n)), ('product with seed + 1', (x * x2).mean(), 1 / np.sqrt(n))]
    keep = S.dropout_mask_np(n, 0.2, seed).mean()
    stats.append(('keep rate - 0.8', keep - 0.8, np.sqrt(0.16 / n)))
    for name, val, sigma in stats:
        print('seed %d %-22s %+.3e = %+.2f sigma' % (seed, name, val, val / sigma))
    for name, val, sigma in stats:
        assert abs(val) <= 4 * sigma, (name, val, sigma)
    assert np.abs(x).max() <= S.NORMAL_MAX
    assert S.dropout_mask_np(1000, 0.0, seed).all()


def test_generator_is_a_pure_function_of_seed_and_counter():
    a, b = S.dropout_mask_np(1000, 0.2, 99), S.dropout_mask_np(70000, 0.2, 99)
    assert np.array_equal(a, b[:1000])
    assert not np.array_equal(S.dropout_mask_np(1000, 0.2, 100), a)
    # the reference value of the splitmix64 finaliser's first outputs (seed 0: z = counter): a known-answer anchor
    z = np.arange(3, dtype=np.uint64)
    py = []
    for i in range(3):
        v = (i + 0x9E3779B97F4A7C15) & S._M64
        v = ((v ^ (v >> 30)) * 0xBF58476D1CE4E5B9) & S._M64
        v = ((v ^ (v >> 27)) * 0x94D049BB133111EB) & S._M64
        py.append((v ^ (v >> 31)) >> 32)
    assert S.mix32(z).tolist() == py


# ---------------------------------------------------------------------------------------------------------------
# argument statuses: every call returns before its first HIP call (read from the sources); nothing is launched
# ---------------------------------------------------------------------------------------------------------------
A = 4096        # a "pointer": 16-byte aligned, never dereferenced
OFF4 = 4100     # 4 bytes off a 16-byte boundary

STATUS_CASES = [
    ('bts_loss_sums C = 9', 'bts_loss_sums', (A, A, A, A, A, A, A, 1 << 20, 1, 64, 9, 9, 9, 2, 2, 2, 8, None), -1),
    ('bts_loss_sums N = 0', 'bts_loss_sums', (A, A, A, A, A, A, A, 1 << 20, 0, 64, 3, 3, 3, 2, 2, 2, 8, None), -1),
    ('bts_loss_sums short workspace', 'bts_loss_sums', (A, A, A, A, A, A, A, 64, 1, 64, 3, 3, 3, 2, 2, 2, 8, None), -4),
    ('bts_loss_bwd C = 0', 'bts_loss_bwd', (A, A, A, A, A, A, None, A, A, A, 1, 64, 0, 3, 3, 2, 2, 2, 8, 1, None), -1),
    ('bts_dice_metric_sums V % W != 0', 'bts_dice_metric_sums', (A, A, A, A, 1, 65, 8, 3, 3, 3, 1, None), -1),
    ('bts_dice_metric_sums table over 60 KB', 'bts_dice_metric_sums', (A, A, A, A, 1, 1000, 1000, 3, 3, 3, 1, None), -3),
    ('bts_l2_reg_fwd nranges = 129', 'bts_l2_reg_fwd', (A, A, A, A, 129, A, A, 1 << 20, None), -1),
    ('bts_l2_reg_fwd nranges = -1', 'bts_l2_reg_fwd', (A, A, A, A, -1, A, A, 1 << 20, None), -1),
    ('bts_l2_reg_fwd short workspace, 0 ranges', 'bts_l2_reg_fwd', (A, A, A, A, 0, A, A, 8, None), -4),
    ('bts_adam_tf_step n = 0', 'bts_adam_tf_step', (A, A, A, A, 0, 1e-4, 0.9, 0.999, 1e-7, 1.0, None), -1),
    ('bts_adam_tf_step pointer 4 bytes off', 'bts_adam_tf_step', (A, A, OFF4, A, 8, 1e-4, 0.9, 0.999, 1e-7, 1.0, None), -2),
    ('bts_adam_tf_step_guarded skip == NULL', 'bts_adam_tf_step_guarded', (A, A, A, A, 8, 1e-4, 0.9, 0.999, 1e-7, 1.0, None, None), -1),
    ('bts_grad_nonfinite flag == NULL', 'bts_grad_nonfinite', (A, 8, None, None), -1),
    ('bts_grad_nonfinite misaligned g', 'bts_grad_nonfinite', (OFF4, 8, A, None), -2),
    ('bts_dropout_apply rate = 1', 'bts_dropout_apply', (A, A, A, 8, 1.0, None), -1),
    ('bts_add_strided ldd < C', 'bts_add_strided', (A, A, 4, 8, 7, 8, 0, None), -1),
    ('bts_dense_fwd N = 0', 'bts_dense_fwd', (A, A, A, A, A, 1 << 20, 0, 8, 8, 0, None), -1),
    ('bts_dense_fwd short workspace', 'bts_dense_fwd', (A, A, A, A, A, 64, 1, 8, 8, 0, None), -4),
    ('bts_colsum C = 4097', 'bts_colsum', (A, A, A, 1 << 30, 1, 8, 4097, 4097, 1.0, 0, 0, None), -1),
    ('bts_colsum ld < C', 'bts_colsum', (A, A, A, 1 << 30, 1, 8, 8, 7, 1.0, 0, 0, None), -1),
    ('bts_colsum short workspace', 'bts_colsum', (A, A, A, 64, 1, 8, 8, 8, 1.0, 0, 0, None), -4),
    ('bts_channel_moments C = 17', 'bts_channel_moments', (A, A, A, A, 1 << 20, 64, 17, 17, None), -1),
    ('bts_channel_moments NULL workspace', 'bts_channel_moments', (A, A, A, None, 1 << 20, 64, 2, 2, None), -4),
    ('bts_augment_crop window outside the volume', 'bts_augment_crop',
     (A, A, A, A, A, 8, 8, 8, 2, 4, 4, 4, 0, 5, 0, 0, A, A, 3, None), -1),
    ('bts_augment_crop flip_mask = 8', 'bts_augment_crop', (A, A, A, A, A, 8, 8, 8, 2, 4, 4, 4, 0, 0, 0, 8, A, A, 3, None), -1),
    ('bts_flip_affine mean without std', 'bts_flip_affine', (A, A + 64, A, None, 1, 2, 2, 2, 2, 0, 1.0, 0, None), -1),
    ('bts_tta_finish C = 251', 'bts_tta_finish', (A, A, A, A, 8, 251, 0.5, None), -1),
    ('bts_vae_sample_fwd L = 0', 'bts_vae_sample_fwd', (A, A, A, 2, 0, None), -1),
    ('bts_fill n = 0', 'bts_fill', (A, 0, 1.0, None), 0),
    ('bts_axpy n = 0', 'bts_axpy', (A, A, 0, 1.0, None), 0),
    ('bts_relu_bwd n = 0', 'bts_relu_bwd', (A, A, A, 0, None), 0),
]


@pytest.mark.parametrize('what,name,args,status', STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_argument_status(what, name, args, status):
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    assert len(args) == len(L.protos[name][1]), 'argument list does not match the header'
    assert getattr(L, '_' + name)(*args) == status
