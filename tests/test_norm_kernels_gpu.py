"""-m gpu: the fp32 GroupNorm kernels (csrc/groupnorm.hip), the gate kernels of csrc/se.hip (bts_se_mlp_fwd, bts_block_epilogue_fwd,
bts_se_bwd) and the fused block backward (csrc/block_bwd.hip) against the fp64 references of tests/norm_ref.py, at the shapes that
reach each path of their host code, with norm_ref's bounds unchanged (tests/test_norm_kernels_host.py shows on the CPU that the
restatements of the documented formulas stay within a quarter of them).  Each case runs its kernels once and prints the ratios it
measured (pytest -s): the fraction of the bound, limit 1."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import norm_ref as N  # noqa: E402

SENTINEL = -7.25
MODES = [N.SLAB, N.CHANNEL]


def dev():
    return torch.device('cuda:0')


def g5(t, dims):
    """(N, V, C) on the CPU -> dense [N, D, H, W, C] on the GPU"""
    return t.reshape((t.shape[0],) + tuple(dims) + (t.shape[-1],)).contiguous().to(dev())


def cpu3(t):
    """[N, D, H, W, C] (any view) on the GPU -> (N, V, C) on the CPU"""
    return t.detach().cpu().reshape(t.shape[0], -1, t.shape[-1])


def sliced(t5, pad, off):
    """a copy of t5 as a channel slice [off, off + C) of a wider slab (row stride C + pad) filled with SENTINEL -> slab, view"""
    c = t5.shape[-1]
    slab = torch.full(t5.shape[:-1] + (c + pad,), SENTINEL, device=t5.device)
    view = slab[..., off:off + c]
    view.copy_(t5)
    return slab, view


def assert_rest_unchanged(slab, c, off, what):
    rest = torch.cat([slab[..., :off], slab[..., off + c:]], -1)
    assert torch.equal(rest, torch.full_like(rest, SENTINEL)), '%s: the kernel wrote outside its channel slice' % what


def gn_run(shape, mode, relu, kind='wide', pad=0, off=0, accumulate=False):
    from bts_amd import ops
    n, dims, c, g = shape
    x, dy, gamma, beta = N.gn_inputs(shape, mode, kind)
    tag = '%s mode %d relu %d %s ld C+%d acc %d' % (shape, mode, relu, kind, pad, accumulate)
    D = dev()
    xg, gam, bet = g5(x, dims), gamma.to(D), beta.to(D)
    mean, rstd = ops.gn_stats(xg, g, mode, N.GN_EPS)
    st = N.gn_stats_ref(x, g, mode)
    N.check(mean, st['mean'], st['b_mean'], 1.0, 'gn_stats mean ' + tag)
    N.check(rstd, st['rstd'], st['b_rstd'], 1.0, 'gn_stats rstd ' + tag)
    mc, rc = mean.cpu(), rstd.cpu()
    assert torch.isfinite(rc).all()
    if pad:
        yslab, yv = sliced(torch.zeros_like(xg), pad, off)
        dslab, dyv = sliced(g5(dy, dims), pad, off)
    else:
        yv, dyv = torch.full_like(xg, SENTINEL), g5(dy, dims)
    ops.gn_apply(xg, gam, bet, mean, rstd, g, mode, relu, out=yv)
    y_r, b_y, _ = N.gn_apply_ref(x, gamma, beta, mc, rc, g, mode, relu)
    N.check(cpu3(yv), y_r, b_y, 1.0, 'gn_apply ' + tag)
    old = [torch.randn(c, generator=N._gen(31 + i)) for i in range(2)]
    dgam, dbet = old[0].to(D), old[1].to(D)
    dx = ops.gn_bwd(xg, dyv, gam, bet, mean, rstd, dgam, dbet, g, mode, relu, accumulate_params=accumulate)
    ref = N.gn_bwd_ref(x, dy, gamma, beta, mc, rc, g, mode, relu, *(old if accumulate else (None, None)))
    assert float(ref['undecided'].double().mean()) <= N.UNDECIDED_CAP
    assert torch.isfinite(dx).all()
    N.check_either(cpu3(dx), ref['dx'], ref['dx_alt'], ref['b_dx'], 'gn_bwd dx ' + tag)
    N.check(dgam, ref['dgamma'], ref['b_dgamma'], 1.0, 'gn_bwd dgamma ' + tag)
    N.check(dbet, ref['dbeta'], ref['b_dbeta'], 1.0, 'gn_bwd dbeta ' + tag)
    if pad:
        assert_rest_unchanged(yslab, c, off, 'gn_apply ' + tag)
        assert_rest_unchanged(dslab, c, off, 'gn_bwd ' + tag)
    return rc, dx


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', N.GN_SHAPES + [N.GN_SHAPE_GENERIC_CAP, N.GN_SHAPE_BLOCK_CAP], ids=str)
def test_groupnorm(shape, mode, relu):
    gn_run(shape, mode, relu)


@pytest.mark.parametrize('relu', [0, 1])
def test_groupnorm_past_the_vectorised_block_cap(relu):
    """channel mode only: in slab mode this shape takes the streaming kernels, whose grid is not capped"""
    gn_run(N.GN_SHAPE_VECTOR_CAP, N.CHANNEL, relu)


@pytest.mark.parametrize('pad,off', [(16, 8), (2, 1)], ids=['ld=C+16', 'ld=C+2'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [N.GN_SHAPE_RAGGED, N.GN_SHAPE_STREAM], ids=str)
def test_groupnorm_views(shape, mode, pad, off):
    """y and dy as channel slices of wider slabs: ld = C + 16 stays on the vectorised / streaming kernels, ld = C + 2 takes the generic
    ones on a vectorisable shape; the rest of each slab is bit-unchanged"""
    gn_run(shape, mode, 1, pad=pad, off=off)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [N.GN_SHAPE_RAGGED, N.GN_SHAPE_STREAM, (2, (4, 4, 4), 2, 2), (1, (2, 2, 2), 1024, 2)], ids=str)
def test_groupnorm_accumulates_onto_nonzero_gradients(shape, mode):
    gn_run(shape, mode, 1, accumulate=True)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [N.GN_SHAPE_RAGGED, N.GN_SHAPE_STREAM], ids=str)
def test_groupnorm_offset_input(shape, mode):
    """8 + 0.5 randn: E[x^2] - mean^2 cancels five digits; the bound charges it"""
    gn_run(shape, mode, 1, kind='offset')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', N.GN_CONSTANT_SHAPES, ids=str)
def test_groupnorm_constant_volume(shape, mode):
    """var = 0, and below 0 where the fp32 squares round down: the clamp.  rstd finite and within its bound of 1 / sqrt(eps), dx finite"""
    rstd, dx = gn_run(shape, mode, 1, kind='constant')
    assert torch.isfinite(rstd).all() and torch.isfinite(dx).all()
    assert float(rstd.max()) <= 1.0 / N.f32(N.GN_EPS) ** 0.5 * (1 + 2 * N.EPS32)


# ---------------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,f,r', N.MLP_SHAPES + [(s[0], s[2], s[3]) for s in N.GATE_SHAPES], ids=str)
def test_se_mlp_fwd(n, f, r):
    from bts_amd import ops
    gen = N._gen(77)
    gap = torch.randn((n, f), generator=gen)
    w1 = torch.randn((f, r), generator=gen) / f ** 0.5
    w2 = torch.randn((r, f), generator=gen) * 2.0 / r ** 0.5
    h_r, b_h, ch_r, b_ch = N.se_mlp_ref(gap, w1, w2)
    D = dev()
    h, ch = ops.se_mlp_fwd(gap.to(D), w1.to(D), w2.to(D))
    N.check(h, h_r, b_h, 1.0, 'se_mlp h (%d,%d,%d)' % (n, f, r))
    N.check(ch, ch_r, b_ch, 1.0, 'se_mlp ch (%d,%d,%d)' % (n, f, r))


def se_bwd_raw(dout, res, sp, gap, h, ch, w1, w2, wsp, dw1, dw2, dwsp, accumulate):
    """ops.se_bwd with the ds and dgap buffers kept: they are outputs of the kernel too"""
    from bts_amd import ops
    from bts_amd._lib import lib
    n, f = res.shape[0], res.shape[4]
    v = res.shape[1] * res.shape[2] * res.shape[3]
    r = w1.shape[1]
    nb = lib().query('bts_se_bwd_workspace', n, v, f, r)
    ws = ops.workspace(nb, res.device)
    dres = torch.full_like(res, SENTINEL)
    ds = torch.full((n * v,), SENTINEL, device=res.device)
    dgap = torch.full((n, f), SENTINEL, device=res.device)
    p = ops._p
    lib().call('bts_se_bwd', p(dout), p(res), p(sp), p(gap), p(h), p(ch), p(w1), p(w2), p(wsp), p(dres), p(ds), p(dgap), p(dw1), p(dw2),
               p(dwsp), p(ws), nb, n, v, f, r, ops.ld_of(dout), 1 if accumulate else 0, ops._stream())
    return dict(dres=dres, ds=ds, dgap=dgap, dw1=dw1, dw2=dw2, dwsp=dwsp)


def check_gate_outputs(got, ref, n, v, f, tag):
    for k in N.GATE_OUTPUTS:
        t = got[k].detach().cpu()
        t = t.reshape(n, v, f) if k == 'dres' else (t.reshape(n, v) if k == 'ds' else t)
        N.check(t, ref[k], ref['b_' + k], 1.0, 'se_bwd %s %s' % (k, tag))


# (conv branch, out as a slice, dout as a slice, accumulate)
GATE_VARIANTS = [(True, False, False, False), (False, True, True, True), (True, True, False, True), (False, False, True, False)]


def gate_run(shape, mode, variant):
    from bts_amd import ops
    conv, out_slice, dout_slice, accumulate = variant
    n, dims, f, r, g = shape
    v = N.nvox(dims)
    D = dev()
    tag = '%s mode %d conv %d slices %d%d acc %d' % (shape, mode, conv, out_slice, dout_slice, accumulate)
    p = N.gate_inputs(shape)
    w1, w2, wsp, gamma, beta = [p[k].to(D) for k in ('w1', 'w2', 'wsp', 'gamma', 'beta')]
    res, c2 = g5(p['res'], dims), g5(p['c2'], dims)
    gap = ops.colsum(res, scale=1.0 / v)
    h, ch = ops.se_mlp_fwd(gap, w1, w2)
    h_r, b_h, ch_r, b_ch = N.se_mlp_ref(gap.cpu(), p['w1'], p['w2'])
    N.check(h, h_r, b_h, 1.0, 'se_mlp h ' + tag)
    N.check(ch, ch_r, b_ch, 1.0, 'se_mlp ch ' + tag)
    mean, rstd = ops.gn_stats(c2, g, mode, N.GN_EPS)
    if out_slice:
        oslab, out = sliced(torch.zeros_like(res), 16, 8)
    else:
        out = torch.full_like(res, SENTINEL)
    sp = ops.block_epilogue_fwd(res, c2 if conv else None, out, wsp, ch, gamma, beta, mean, rstd, g, mode)
    sp_r, b_sp, out_r, b_out = N.epilogue_ref(p['res'], p['c2'] if conv else None, p['wsp'], ch.cpu(), p['gamma'], p['beta'], mean.cpu(),
                                              rstd.cpu(), g, mode)
    N.check(sp.cpu().reshape(n, v), sp_r, b_sp, 1.0, 'epilogue sp ' + tag)
    N.check(cpu3(out), out_r, b_out, 1.0, 'epilogue out ' + tag)
    if out_slice:
        assert_rest_unchanged(oslab, f, 8, 'epilogue ' + tag)
    # backward: its own inputs, seam voxels at 8; sp, gap, h, ch are inputs of the kernel
    q = N.gate_inputs(shape, seams='gate')
    resb, dout = g5(q['res'], dims), g5(q['dout'], dims)
    if dout_slice:
        dslab, dout = sliced(dout, 16, 8)
    spb, gapb = q['sp_in'].reshape(-1).to(D), q['gap_in'].to(D)
    hb, chb = ops.se_mlp_fwd(gapb, w1, w2)
    names = (('dw1', 'w1'), ('dw2', 'w2'), ('dwsp', 'wsp'))
    old = dict((k, torch.randn(q[w].shape, generator=N._gen(5))) for k, w in names)
    bufs = dict((k, old[k].to(D)) for k, _ in names)
    got = se_bwd_raw(dout, resb, spb, gapb, hb, chb, w1, w2, wsp, bufs['dw1'], bufs['dw2'], bufs['dwsp'], accumulate)
    ref = N.se_bwd_ref(q['dout'], q['res'], q['sp_in'], q['gap_in'], hb.cpu(), chb.cpu(), q['w1'], q['w2'], q['wsp'],
                       old=old if accumulate else None)
    check_gate_outputs(got, ref, n, v, f, tag)
    if dout_slice:
        assert_rest_unchanged(dslab, f, 8, 'se_bwd ' + tag)


@pytest.mark.parametrize('variant', GATE_VARIANTS, ids=lambda t: 'conv%d-out%d-dout%d-acc%d' % tuple(int(b) for b in t))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', N.GATE_SHAPES, ids=str)
def test_gate_epilogue_and_backward(shape, mode, variant):
    gate_run(shape, mode, variant)


@pytest.mark.parametrize('mode,variant', [(N.SLAB, GATE_VARIANTS[0]), (N.CHANNEL, GATE_VARIANTS[1])], ids=['slab-dense', 'channel-slices'])
def test_gate_past_the_block_caps(mode, variant):
    gate_run(N.GATE_SHAPE_CAP, mode, variant)


# ---------------------------------------------------------------------------------------------------------------
# the fused block backward, and the two-kernel route on the same tensors, both against the fp64 references
# ---------------------------------------------------------------------------------------------------------------
def block_bwd_raw(dout, res, c2, sp, gap, h, ch, w1, w2, wsp, gamma, beta, mean, rstd, groups, bufs, acc_gate, acc_norm):
    from bts_amd import ops
    from bts_amd._lib import lib
    n, f = res.shape[0], res.shape[4]
    v = res.shape[1] * res.shape[2] * res.shape[3]
    r = w1.shape[1]
    assert ops.block_bwd_takes(res, r, groups, dout, c2)
    nb = lib().query('bts_block_bwd_workspace', n, v, f, r, groups)
    ws = ops.workspace(nb, res.device)
    dres, dc2 = torch.full_like(res, SENTINEL), torch.full_like(c2, SENTINEL)
    ds = torch.full((n * v,), SENTINEL, device=res.device)
    dgap = torch.full((n, f), SENTINEL, device=res.device)
    p = ops._p
    lib().call('bts_block_bwd', p(dout), ops.ld_of(dout), p(res), p(c2), p(sp), p(gap), p(h), p(ch), p(w1), p(w2), p(wsp), p(gamma), p(beta),
               p(mean), p(rstd), p(dres), p(dc2), p(ds), p(dgap), p(bufs['dw1']), p(bufs['dw2']), p(bufs['dwsp']), p(bufs['dgamma']),
               p(bufs['dbeta']), p(ws), nb, n, v, f, r, groups, 1 if acc_gate else 0, 1 if acc_norm else 0, ops._stream())
    return dict(dres=dres, ds=ds, dgap=dgap, dw1=bufs['dw1'], dw2=bufs['dw2'], dwsp=bufs['dwsp']), dc2


# (dout as a slice, accumulate the gate's parameter gradients, accumulate GroupNorm's)
BLOCK_VARIANTS = [(False, False, True), (False, True, False), (True, False, False), (True, True, True)]


@pytest.mark.parametrize('variant', BLOCK_VARIANTS, ids=lambda t: 'slice%d-gate%d-norm%d' % tuple(int(b) for b in t))
@pytest.mark.parametrize('shape', N.BLOCK_SHAPES + [N.BLOCK_SHAPE_CAP], ids=str)
def test_fused_block_backward(shape, variant):
    from bts_amd import ops
    dout_slice, acc_gate, acc_norm = variant
    n, dims, f, r, g = shape
    v = N.nvox(dims)
    D = dev()
    tag = '%s slice %d acc %d%d' % (shape, dout_slice, acc_gate, acc_norm)
    q = N.gate_inputs(shape, seams='blk')
    w1, w2, wsp, gamma, beta = [q[k].to(D) for k in ('w1', 'w2', 'wsp', 'gamma', 'beta')]
    res, c2, dout = g5(q['res'], dims), g5(q['c2'], dims), g5(q['dout'], dims)
    if dout_slice:
        dslab, dout = sliced(dout, 16, 8)
    sp, gap = q['sp_in'].reshape(-1).to(D), q['gap_in'].to(D)
    h, ch = ops.se_mlp_fwd(gap, w1, w2)
    mean, rstd = ops.gn_stats(c2, g, N.SLAB, N.GN_EPS)
    names = (('dw1', 'w1'), ('dw2', 'w2'), ('dwsp', 'wsp'), ('dgamma', 'gamma'), ('dbeta', 'beta'))
    old = dict((k, torch.randn(q[w].shape, generator=N._gen(6))) for k, w in names)
    gn = N.gn_bwd_ref(q['c2'], q['dout'], q['gamma'], q['beta'], mean.cpu(), rstd.cpu(), g, N.SLAB, 1,
                      old['dgamma'] if acc_norm else None, old['dbeta'] if acc_norm else None)
    assert float(gn['undecided'].double().mean()) <= N.UNDECIDED_CAP
    se = N.se_bwd_ref(q['dout'], q['res'], q['sp_in'], q['gap_in'], h.cpu(), ch.cpu(), q['w1'], q['w2'], q['wsp'], old=old if acc_gate else None)

    def hold(route, gate, dc2, bufs):
        check_gate_outputs(gate, se, n, v, f, '%s %s' % (route, tag))
        N.check_either(cpu3(dc2), gn['dx'], gn['dx_alt'], gn['b_dx'], '%s dc2 %s' % (route, tag))
        N.check(bufs['dgamma'], gn['dgamma'], gn['b_dgamma'], 1.0, '%s dgamma %s' % (route, tag))
        N.check(bufs['dbeta'], gn['dbeta'], gn['b_dbeta'], 1.0, '%s dbeta %s' % (route, tag))

    bufs = dict((k, old[k].to(D)) for k, _ in names)
    gate, dc2 = block_bwd_raw(dout, res, c2, sp, gap, h, ch, w1, w2, wsp, gamma, beta, mean, rstd, g, bufs, acc_gate, acc_norm)
    hold('block_bwd', gate, dc2, bufs)
    bufs = dict((k, old[k].to(D)) for k, _ in names)
    gate = se_bwd_raw(dout, res, sp, gap, h, ch, w1, w2, wsp, bufs['dw1'], bufs['dw2'], bufs['dwsp'], acc_gate)
    dc2 = ops.gn_bwd(c2, dout, gamma, beta, mean, rstd, bufs['dgamma'], bufs['dbeta'], g, N.SLAB, True, accumulate_params=acc_norm)
    hold('two-kernel', gate, dc2, bufs)
    if dout_slice:
        assert_rest_unchanged(dslab, f, 8, 'block_bwd ' + tag)
