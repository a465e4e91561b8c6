"""-m gpu: the kernels that close the training step -- loss, metric, L2, Adam and its overflow guard, the Dense layers, column sums,
channel moments and the element-wise pieces -- against the fp64 references of tests/step_ref.py, at the edges where such kernels go
wrong: C = 1 and C = LOSS_MAXC, channel-slice views, NULL options, n % 4 tails, and one case just past every grid cap (the second
trip of the grid-stride loop).  The tolerances are step_ref's bounds with step_ref's K, unchanged; each check prints its measured
ratio before it asserts (pytest -s).  Outputs that are channel slices of a wider slab carry a sentinel in the other channels.
No test passes a pointer or an extent that lets a kernel touch memory outside its buffers."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import step_ref as S  # noqa: E402

SENTINEL = 7.0
EW_SIZES = [1, 255, 256, 257, 2097152 + 257]      # the last: past the 8192-block cap of the element-wise grids


def dev():
    return torch.device('cuda:0')


def ops_():
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


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------------------------
def run_loss(tensors, gs, ts):
    """tensors: device views (p, y, x, yv, proj) or (p, y, None, None, None) -> sums, value, parts, dlogit, dyvae, dproj"""
    ops = ops_()
    p, y, x, yv, proj = tensors
    c = p.shape[-1]
    sums = ops.loss_sums(p, y, x, yv, proj)
    val, parts = ops.loss_value(sums, c, has_vae=x is not None)
    gsc = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=dev())
    dl = torch.full(p.shape, SENTINEL, device=dev())
    dyv = torch.full(x.shape, SENTINEL, device=dev()) if x is not None else None
    dpr = torch.full(proj.shape, SENTINEL, device=dev()) if x is not None else None
    ops.loss_bwd(p, y, x, yv, proj, sums, gsc, dl, dyv, dpr, through_sigmoid=bool(ts))
    return sums.cpu(), float(val), parts.cpu(), dl, dyv, dpr


def check_loss(out, ref, c, lz, what, vae=True):
    sums, val, parts, dl, dyv, dpr = out
    for k, name in enumerate('IPT'):
        S.check(sums[k * c:(k + 1) * c], ref[name], S.EPS32 * ref[name], 1.0, what + ' sums ' + name)
    print('%s value: err %.3e, bound %.3e' % (what, abs(val - ref['loss']), ref['value_bound']))
    assert abs(val - ref['loss']) <= ref['value_bound']
    assert abs(float(parts[0]) - ref['dice']) <= 4 * S.EPS32
    S.check(dl, ref['dlogit'], ref['B_dlogit'], S.K_LOSS_GRAD, what + ' dlogit')
    if vae:
        assert float(sums[3 * c + 2]) == ref['numel_x'] and float(sums[3 * c + 3]) == ref['numel_z']
        assert abs(float(sums[3 * c]) - ref['sq']) <= 4 * S.EPS32 * ref['sq']
        assert abs(float(sums[3 * c + 1]) - ref['klsum']) <= 4 * S.EPS32 * ref['klabs']
        assert abs(float(parts[1]) - ref['l2']) <= 4 * S.EPS32 * ref['l2']
        assert abs(float(parts[2]) - ref['kl']) <= 4 * S.EPS32 * ref['klabs'] / ref['numel_z']
        S.check(dyv, ref['dyvae'], ref['B_dyvae'], S.K_LOSS_GRAD, what + ' dyvae')
        S.check(dpr[:, :lz], ref['dproj'][:, :lz], ref['B_dproj'][:, :lz], S.K_LOSS_GRAD, what + ' dproj mean')
        S.check(dpr[:, lz:], ref['dproj'][:, lz:], ref['B_dproj'][:, lz:], S.K_LOSS_GRAD, what + ' dproj logvar')
    else:
        assert float(parts[1]) == 0.0 and float(parts[2]) == 0.0
        assert abs(val - ref['dice']) <= 4 * S.EPS32


@pytest.mark.parametrize('shape', S.LOSS_SHAPES_SMALL)
@pytest.mark.parametrize('ts', [1, 0])
@pytest.mark.parametrize('gs', [None, 0.125, 65536.0])
def test_loss_small(shape, ts, gs):
    n, dims, c, cx, lz = shape
    host = S.loss_inputs(n, dims, c, cx, lz)
    ref = S.loss_ref(*host, gs=1.0 if gs is None else gs, through_sigmoid=ts)
    proj = host[4].to(dev())
    check_loss(run_loss([t.to(dev()) for t in host], gs, ts), ref, c, lz, 'dense')
    for off in (0, 5):      # y_pred, y, x, y_vae as channel slices of wider slabs
        slabs = [on_slab(t, off) for t in host[:4]]
        check_loss(run_loss([v for _, v in slabs] + [proj], gs, ts), ref, c, lz, 'slice at %d' % off)
        for (sl, v) in slabs:
            assert sentinel_intact(sl, off, v.shape[-1])
    # without a VAE: the Dice part alone
    ref0 = S.loss_ref(host[0], host[1], gs=1.0 if gs is None else gs, through_sigmoid=ts)
    check_loss(run_loss([host[0].to(dev()), host[1].to(dev()), None, None, None], gs, ts), ref0, c, lz, 'no vae', vae=False)


@pytest.mark.parametrize('shape', [S.LOSS_SHAPE_PAST_PARTIAL, S.LOSS_SHAPE_PAST_BWD], ids=['past_loss_partial_cap', 'past_loss_bwd_cap'])
def test_loss_past_the_grid_caps(shape):
    n, dims, c, cx, lz = shape
    host = S.loss_inputs(n, dims, c, cx, lz)
    ref = S.loss_ref(*host, gs=1.0, through_sigmoid=1)
    check_loss(run_loss([t.to(dev()) for t in host], None, 1), ref, c, lz, 'large')


@pytest.mark.parametrize('shape,cut', [(S.LOSS_SHAPES_SMALL[0], 1), (S.LOSS_SHAPES_SMALL[1], 1), (S.LOSS_SHAPES_SMALL[2], 1)])
def test_loss_shard_additivity(shape, cut):
    """the data-parallel contract of the header: the raw sums of two shards add up to the batch's; each shard's gradient rows
    follow from the summed sums"""
    ops = ops_()
    n, dims, c, cx, lz = shape
    host = S.loss_inputs(n, dims, c, cx, lz)
    ref = S.loss_ref(*host, gs=1.0, through_sigmoid=1)
    parts = [[t[:cut].contiguous().to(dev()) for t in host], [t[cut:].contiguous().to(dev()) for t in host]]
    sums = ops.loss_sums(*parts[0]) + ops.loss_sums(*parts[1])
    val, _ = ops.loss_value(sums, c)
    assert abs(float(val) - ref['loss']) <= ref['value_bound']
    lo = 0
    for sh in parts:
        p, y, x, yv, proj = sh
        dl, dyv, dpr = torch.empty_like(p), torch.empty_like(x), torch.empty_like(proj)
        ops.loss_bwd(p, y, x, yv, proj, sums, None, dl, dyv, dpr, through_sigmoid=True)
        hi = lo + p.shape[0]
        S.check(dl, ref['dlogit'][lo:hi], ref['B_dlogit'][lo:hi], S.K_LOSS_GRAD, 'shard dlogit')
        S.check(dyv, ref['dyvae'][lo:hi], ref['B_dyvae'][lo:hi], S.K_LOSS_GRAD, 'shard dyvae')
        S.check(dpr, ref['dproj'][lo:hi], ref['B_dproj'][lo:hi], S.K_LOSS_GRAD, 'shard dproj')
        lo = hi


# ---------------------------------------------------------------------------------------------------------------
# metric
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', S.METRIC_SHAPES)
@pytest.mark.parametrize('channels_last_axes', [True, False])
def test_dice_metric(shape, channels_last_axes):
    ops = ops_()
    n, dims, c = shape
    yt, yp = S.metric_inputs(n, dims, c)
    top = yp.max(-1).values
    assert bool((top == 0.5).any()), 'no exact 0.5 maximum in the inputs'
    if c > 1:
        assert bool(((yp == top.unsqueeze(-1)).sum(-1) > 1).any()), 'no tie in the inputs'
        assert bool((yp.min(-1).values == top).any()), 'no all-equal row in the inputs'
    macro, micro, labels, table = S.metric_ref(yt, yp, channels_last_axes)
    for layout in ('dense', 'slab'):
        if layout == 'dense':
            ytg, ypg = yt.to(dev()), yp.to(dev())
        else:
            (_, ytg), (_, ypg) = on_slab(yt, 5), on_slab(yp, 3)
        for want in (True, False):
            tab, lab = ops.dice_metric_sums(ytg, ypg, channels_last_axes, want_labels=want)
            assert torch.equal(tab.cpu(), table), 'the table holds counts: exact'
            if want:
                assert torch.equal(lab.cpu(), labels), 'label map must be bit-exact'
            mv = ops.dice_metric_value(tab, dims[2], c, channels_last_axes).cpu()
            assert abs(float(mv[0]) - macro) <= 2 * S.EPS32 and abs(float(mv[1]) - micro) <= 2 * S.EPS32, (mv, macro, micro)


def test_dice_metric_empty_prediction_and_truth():
    ops = ops_()
    yp = torch.full((1, 3, 4, 5, 3), 0.25)
    yt = torch.zeros((1, 3, 4, 5, 3))
    macro, micro, labels, table = S.metric_ref(yt, yp, True)
    tab, lab = ops.dice_metric_sums(yt.to(dev()), yp.to(dev()), True)
    mv = ops.dice_metric_value(tab, 5, 3, True).cpu()
    assert np.isnan(micro) and bool(torch.isnan(mv[1])) and float(mv[0]) == macro == 1.0
    assert int(lab.max()) == 0 and float(tab.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# L2
# ---------------------------------------------------------------------------------------------------------------
def _l2_cases():
    many, off = [], 2
    for i in range(128):
        ln = (i * 37) % 50 if i % 9 else 0
        many.append((off, ln, 1e-5 * (1 + i % 3)))
        off += ln + 3
    return {'none': [], 'one_of_1': [(3, 1, 1e-5)], 'many_128': many, 'past_caps': [(17, 600001, 2e-5)]}


@pytest.mark.parametrize('case', ['none', 'one_of_1', 'many_128', 'past_caps'])
@pytest.mark.parametrize('gs', [None, 65536.0])
def test_l2(case, gs):
    ops = ops_()
    ranges = _l2_cases()[case]
    n = max([o + l for o, l, _ in ranges] + [16]) + 5
    g0 = torch.Generator().manual_seed(50)
    p, g = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    val, vb, gr, B = S.l2_ref(p, g, ranges, 1.0 if gs is None else gs)
    pg, gg = p.to(dev()), g.to(dev())
    got = float(ops.l2_reg_fwd(pg, ranges))
    print('l2 value err %.3e bound %.3e' % (abs(got - val), vb))
    assert abs(got - val) <= vb
    gsc = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=dev())
    ops.l2_reg_bwd(pg, gg, ranges, gsc)
    S.check(gg, gr, B, S.K_L2_GRAD, 'l2 grad')
    inside = torch.zeros(n, dtype=torch.bool)
    for o, l, _ in ranges:
        inside[o:o + l] = True
    assert same_bits(gg.cpu()[~inside], g[~inside]), 'gradient outside the ranges must stay bit-identical'
    if not ranges:
        assert got == 0.0


# ---------------------------------------------------------------------------------------------------------------
# Adam, the guard, the overflow flag
# ---------------------------------------------------------------------------------------------------------------
ADAM_SIZES = [1, 3, 4, 5, 1023, 10007, 4194304 + 1203]        # the last: past the 4096-block cap


@pytest.mark.parametrize('n', ADAM_SIZES)
@pytest.mark.parametrize('p0', ['zero', 'normal'])
def test_adam(n, p0):
    """p0 = 0 makes the update itself what is compared: that pins epsilon outside the root (step_ref / the host test)"""
    ops = ops_()
    # (the wrap case costs a second of fp64 reference per step: it runs one gmul, the one that is neither 1 nor a power of two away
    # from underflow; the three values run on every other size)
    for gmul in ((1.0, 0.125, 1.0 / 65536) if n < 1000000 else (0.125,)):
        g1 = S.adam_grad(n, 1, gmul)
        p_init = torch.zeros(n) if p0 == 'zero' else torch.randn(n, generator=torch.Generator().manual_seed(5))
        p, m, v = p_init.to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
        for t, g in ((1, g1), (2, g1 * -0.7), (3, g1)):
            sc = S.adam_scalars(t)
            (pr, mr, vr), (Bp, Bm, Bv) = S.adam_ref(p.cpu(), g, m.cpu(), v.cpu(), *sc, gmul)      # re-seeded from the device state
            ops.adam_tf_step(p, g.to(dev()), m, v, *sc, gmul=gmul)
            what = 'adam n=%d gmul=%g step %d ' % (n, gmul, t)
            S.check(p, pr, Bp, S.K_ADAM, what + 'p')
            S.check(m, mr, Bm, S.K_ADAM, what + 'm')
            S.check(v, vr, Bv, S.K_ADAM, what + 'v')
        zero = (g1 == 0)
        assert same_bits(p.cpu()[zero], p_init[zero]) and not bool(m.cpu()[zero].any()) and not bool(v.cpu()[zero].any())
        assert same_bits(m.cpu()[zero], torch.zeros(int(zero.sum()))) and same_bits(v.cpu()[zero], torch.zeros(int(zero.sum())))


@pytest.mark.parametrize('n', [1, 5, 10007])
def test_adam_guarded(n):
    ops = ops_()
    g0 = torch.Generator().manual_seed(6)
    p0, m0 = torch.randn(n, generator=g0), torch.randn(n, generator=g0) * 0.1
    v0 = torch.rand(n, generator=g0) * 0.01
    g = S.adam_grad(n, 2, 1.0).to(dev())
    sc = S.adam_scalars(2)
    plain = [t.to(dev()) for t in (p0, m0, v0)]
    ops.adam_tf_step(plain[0], g, plain[1], plain[2], *sc, gmul=0.5)
    for skip in (0, 1):
        st = [t.to(dev()) for t in (p0, m0, v0)]
        flag = torch.tensor([skip], dtype=torch.int32, device=dev())
        ops.adam_tf_step(st[0], g, st[1], st[2], *sc, gmul=0.5, skip=flag)
        want = plain if skip == 0 else (p0, m0, v0)
        for a, b in zip(st, want):
            assert same_bits(a, b), 'guarded step, skip = %d' % skip
        assert int(flag.item()) == skip


NONFINITE = {'+inf': 0x7f800000, '-inf': -8388608, 'quiet nan': 0x7fc00000, 'signalling nan': 0x7f800001}


@pytest.mark.parametrize('n', [1, 3, 4, 7, 1024, 2097152 + 1027])       # the last: past the 2048-block cap
def test_grad_nonfinite(n):
    ops = ops_()
    g = torch.randn(n, generator=torch.Generator().manual_seed(8))
    edge = torch.tensor([3.4028234663852886e38, 1e-45, -1e-40, -0.0, -3.4028234663852886e38])
    k = min(n, 5)
    g[:k] = edge[:k]
    if n > 8:
        g[-3:] = edge[:3]
    gg = g.to(dev())
    gi = gg.view(torch.int32)
    flag = torch.ones(1, dtype=torch.int32, device=dev())
    ops.grad_nonfinite(gg, flag)
    assert int(flag.item()) == 0, 'largest finite, denormals and -0.0 are finite'
    body = 4 * (n // 4)
    pos = {0, n - 1}
    if body:
        pos.add(body - 1)
    if body < n:
        pos.add(body)
    if n > 2097152:
        pos.add(2097152 + 1)
        pos.add(2097152 + 4 * 200)
    assert max(pos) < n
    for i in sorted(pos):
        for name, pattern in NONFINITE.items():
            keep = int(gi[i].item())
            gi[i] = pattern
            ops.grad_nonfinite(gg, flag)
            assert int(flag.item()) == 1, '%s at %d of %d not seen' % (name, i, n)
            gi[i] = keep
        ops.grad_nonfinite(gg, flag)
        assert int(flag.item()) == 0, 'the next clean call rewrites the flag'


# ---------------------------------------------------------------------------------------------------------------
# Dense
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', S.DENSE_SHAPES)
def test_dense(shape):
    ops = ops_()
    n, fin, fout, relu = shape
    x, w, b, dy = S.dense_inputs(n, fin, fout)
    xg, wg, bg, dyg = [t.to(dev()) for t in (x, w, b, dy)]
    for bias, biasg in ((b, bg), (None, None)):
        ref, B = S.dense_fwd_ref(x, w, bias, relu)
        S.check(ops.dense_fwd(xg, wg, biasg, relu), ref, B, S.K_DENSE, 'dense fwd %s bias=%s' % (shape, bias is not None))
    g0 = torch.Generator().manual_seed(60)
    odx, odw, odb = torch.randn((n, fin), generator=g0), torch.randn((fin, fout), generator=g0), torch.randn((fout,), generator=g0)
    for acc_dx in (0, 1):
        for acc_p in (0, 1):
            (dxr, dwr, dbr), (Bx, Bw, Bb) = S.dense_bwd_ref(x, w, dy, odx if acc_dx else None, odw if acc_p else None,
                                                            odb if acc_p else None)
            dx, dw, db = odx.to(dev()), odw.to(dev()), odb.to(dev())
            ops.dense_bwd(xg, wg, dyg, dx, dw, db, bool(acc_dx), bool(acc_p))
            what = 'dense bwd %s acc_dx=%d acc_p=%d ' % (shape, acc_dx, acc_p)
            S.check(dx, dxr, Bx, S.K_DENSE, what + 'dx')
            S.check(dw, dwr, Bw, S.K_DENSE, what + 'dw')
            S.check(db, dbr, Bb, S.K_DENSE, what + 'db')
    (dxr, dwr, dbr), (Bx, Bw, Bb) = S.dense_bwd_ref(x, w, dy)
    dw, db = odw.to(dev()), odb.to(dev())
    ops.dense_bwd(xg, wg, dyg, None, dw, db)
    S.check(dw, dwr, Bw, S.K_DENSE, 'dense bwd dx=None dw')
    S.check(db, dbr, Bb, S.K_DENSE, 'dense bwd dx=None db')
    dx, dw = odx.to(dev()), odw.to(dev())
    ops.dense_bwd(xg, wg, dyg, dx, dw, None)
    S.check(dx, dxr, Bx, S.K_DENSE, 'dense bwd db=None dx')
    S.check(dw, dwr, Bw, S.K_DENSE, 'dense bwd db=None dw')


# ---------------------------------------------------------------------------------------------------------------
# column sums, channel moments
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [3, 20, 32, 1028])      # 1028: a second column pass; 3, and every slice at channel 1: the scalar path
def test_colsum(c):
    ops = ops_()
    g0 = torch.Generator().manual_seed(70 + c)
    for rows in (1, 63, 64, 1000):
        for n in (1, 3):
            x = torch.randn((n, rows, c), generator=g0)
            old = torch.randn((n, c), generator=g0)
            views = [x.to(dev()), on_slab(x, 0)[1], on_slab(x, 1, extra=9)[1]]       # ld = C, C + 8 (aligned), C + 9 from channel 1
            for xv in views:
                for scale in (1.0, 1.0 / rows):
                    for son in (False, True):
                        for acc in (False, True):
                            o = old[0] if son else old
                            ref, bound = S.colsum_ref(x, scale, son, o if acc else None)
                            out = o.to(dev()).clone()
                            ops.colsum(xv, scale, son, out=out, accumulate=acc)
                            r = S.ratio(out.cpu(), ref, bound)
                            assert r <= 1.0, ('colsum', c, rows, n, xv.stride(), scale, son, acc, r)


@pytest.mark.parametrize('c', [1, 2, 16])
@pytest.mark.parametrize('pad', [0, 3])
def test_channel_moments(c, pad):
    """48x48x64 voxels (past the 512-block cap), mean 1000 and deviation 1: E[x^2] - mean^2 cancels six digits"""
    from bts_amd._lib import lib
    ops = ops_()
    nvox = 48 * 48 * 64
    x = torch.randn((nvox, c), generator=torch.Generator().manual_seed(80 + c)) + 1000.0
    slab, xv = on_slab(x, pad, extra=pad)
    mr, vr, mb, vb = S.moments_ref(x)
    nb = lib().query('bts_channel_moments_workspace', c)
    ws = ops.workspace(nb, dev())
    mean, var = torch.empty(c, device=dev()), torch.empty(c, device=dev())
    lib().call('bts_channel_moments', ops._p(xv), ops._p(mean), ops._p(var), ops._p(ws), nb, nvox, c, c + pad, ops._stream())
    S.check(mean, mr, mb, 1.0, 'moments mean')
    S.check(var, vr, vb, 1.0, 'moments var')
    lib().call('bts_channel_moments', ops._p(xv), None, ops._p(var), ops._p(ws), nb, nvox, c, c + pad, ops._stream())
    S.check(var, vr, vb, 1.0, 'moments var, mean == NULL')


def test_channel_moments_of_a_constant_volume():
    """E[x^2] - mean^2 of a constant is 0 up to the rounding of the fp64 sums, of either sign: the result is exactly 0, never a
    negative number (sqrt(var) feeds the augmentation, train.py:19-21)"""
    ops = ops_()
    nvox = 48 * 48 * 64
    vals = torch.tensor([1000.1 + 0.7 * i for i in range(16)])
    m2, v2 = ops.channel_moments(vals.repeat(nvox, 1).to(dev()))
    print('variance of the constant channels:', v2.cpu().tolist())
    assert same_bits(v2, torch.zeros(16)), 'a constant volume has variance exactly 0'
    assert same_bits(m2, vals)


# ---------------------------------------------------------------------------------------------------------------
# element-wise
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', EW_SIZES)
def test_fill_axpy_relu_bwd(n):
    ops = ops_()
    g0 = torch.Generator().manual_seed(90)
    t = torch.full((n + 2,), SENTINEL, device=dev())
    ops.fill(t[1:n + 1], -1.5)            # an unaligned start: the kernel is scalar
    assert same_bits(t[1:n + 1], torch.full((n,), -1.5)) and float(t[0]) == SENTINEL and float(t[n + 1]) == SENTINEL
    x, y = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    ref, B = S.axpy_ref(y, x, -0.37)
    yg = y.to(dev())
    ops.axpy(yg, x.to(dev()), -0.37)
    S.check(yg, ref, B, S.K_EW, 'axpy n=%d' % n)
    act = torch.relu(y)
    act[::5] = 0.0
    act[1::7] = -0.0
    dx = ops.relu_bwd(act.to(dev()), x.to(dev()))
    assert same_bits(dx, torch.where(act > 0, x, torch.zeros(n)))


@pytest.mark.parametrize('n', EW_SIZES)
@pytest.mark.parametrize('rate', [0.0, 0.2])
def test_dropout_and_normal(n, rate):
    ops = ops_()
    seed = 1234
    mask = ops.dropout_mask((n,), rate, seed, dev())
    want = torch.from_numpy(S.dropout_mask_np(n, rate, seed))
    assert torch.equal(mask.cpu(), want), 'the mask is a pure integer function of (seed, i): bit for bit'
    x = torch.randn(n, generator=torch.Generator().manual_seed(91))
    ref, B = S.dropout_apply_ref(x, want, rate)
    y = ops.dropout_apply(x.to(dev()), mask, rate)
    S.check(y, ref, B, S.K_EW, 'dropout_apply n=%d rate=%g' % (n, rate))
    assert same_bits(y.cpu()[want == 0], torch.zeros(int((want == 0).sum())))
    if rate == 0.0:
        assert same_bits(y, x)
        e = ops.normal((n,), seed, dev()).cpu()
        ref, unit = S.normal_ref(n, seed)
        S.check(e, torch.from_numpy(ref), torch.from_numpy(unit), S.K_NORMAL, 'normal n=%d' % n)
        assert float(e.abs().max()) <= S.NORMAL_MAX


def test_generator_counter_property():
    """element i depends on (seed, i) alone: a short draw is the head of a long one, across the grid wrap"""
    ops = ops_()
    big = EW_SIZES[-1]
    mb, nb = ops.dropout_mask((big,), 0.2, 77, dev()), ops.normal((big,), 77, dev())
    for small in (1, 257, 70000):
        assert torch.equal(ops.dropout_mask((small,), 0.2, 77, dev()), mb[:small])
        assert same_bits(ops.normal((small,), 77, dev()), nb[:small])


@pytest.mark.parametrize('rows,c', [(1, 1), (7, 3), (300, 32)])
@pytest.mark.parametrize('dpad', [0, 5])
@pytest.mark.parametrize('spad', [0, 3])
def test_add_strided_and_sigmoid_bwd(rows, c, dpad, spad):
    ops = ops_()
    from bts_amd._lib import lib
    g0 = torch.Generator().manual_seed(92)
    src, dst0 = torch.randn((rows, c), generator=g0), torch.randn((rows, c), generator=g0)
    sslab, sv = on_slab(src, spad, extra=spad)
    for accumulate in (0, 1):
        dslab, dv = on_slab(dst0, dpad, extra=dpad)
        lib().call('bts_add_strided', ops._p(dv), ops._p(sv), rows, c, c + dpad, c + spad, accumulate, ops._stream())
        assert same_bits(dv, dst0 + src if accumulate else src)
        assert sentinel_intact(dslab, dpad, c)
    y = torch.sigmoid(src * 3)
    yslab, yv = on_slab(y, dpad, extra=dpad)
    dx = torch.full((rows, c), SENTINEL, device=dev())
    lib().call('bts_sigmoid_bwd', ops._p(yv), ops._p(sv), ops._p(dx), rows, c, c + dpad, c + spad, ops._stream())
    ref, B = S.sigmoid_bwd_ref(y, src)
    S.check(dx, ref, B, S.K_EW, 'sigmoid_bwd')


def test_scalar_lincomb():
    ops = ops_()
    a, b = torch.tensor([1.2345678]), torch.tensor([-9.87654e-3])
    for bb in (None, b):
        for ca, cb in ((1.0, 1.0), (0.3, -65536.0)):
            ref, B = S.lincomb_ref(a, bb, ca, cb)
            out = ops.scalar_lincomb(a.to(dev()), None if bb is None else bb.to(dev()), ca, cb)
            S.check(out, ref, B, S.K_EW, 'scalar_lincomb')


@pytest.mark.parametrize('n,lz', [(1, 1), (3, 8), (5, 128)])
def test_vae_sample(n, lz):
    ops = ops_()
    g0 = torch.Generator().manual_seed(93)
    proj, eps, dz, old = [torch.randn(sh, generator=g0) for sh in ((n, 2 * lz), (n, lz), (n, lz), (n, 2 * lz))]
    zr, Bz, dr, Bd = S.vae_sample_ref(proj, eps, dz, old)
    z = ops.vae_sample_fwd(proj.to(dev()), eps.to(dev()))
    S.check(z, zr, Bz, S.K_VAE, 'vae sample fwd')
    dproj = old.to(dev())         # pre-filled: the kernel ADDS into it
    ops.vae_sample_bwd(proj.to(dev()), eps.to(dev()), dz.to(dev()), dproj)
    S.check(dproj, dr, Bd, S.K_VAE, 'vae sample bwd')
