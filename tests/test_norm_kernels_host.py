"""CPU: the bounds tests/test_norm_kernels_gpu.py applies to the fp32 GroupNorm, gate and fused block-backward kernels are honest.

The references of tests/norm_ref.py are pinned to the oracle (oracle/torch_ref.py and autograd), every fp32 restatement stays within
a quarter of the bound its kernel is held to (the bound itself for the bounds without a K), the seam items of the reduction inputs
are each worth 8 bounds, the inputs keep the share of elements with an undecided ReLU mask below norm_ref's cap, and the entry
points of groupnorm.hip, se.hip's gate half and block_bwd.hip turn bad arguments away before any launch.  Each test prints the ratio
it measured (pytest -s)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import norm_ref as N  # noqa: E402

SMALL_GN = list(N.GN_SHAPES)
MODES = [N.SLAB, N.CHANNEL]


def held(what, got, ref, bound, limit=0.25):
    r = N.ratio(got, ref, bound)
    print('%-58s %.3f (limit %g)' % (what, r, limit))
    assert r <= limit, '%s: the fp32 restatement is %.3f of its bound, limit %g' % (what, r, limit)
    return r


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------
# the references against the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SMALL_GN, ids=str)
def test_statistics_and_apply_compose_to_the_oracle(shape, mode):
    n, dims, c, g = shape
    x, _, gamma, beta = N.gn_inputs(shape, mode)
    st = N.gn_stats_ref(x, g, mode, abi_eps=False)
    y, _, _ = N.gn_apply_ref(x, gamma, beta, st['mean'], st['rstd'], g, mode, 0)
    want = N.group_norm_oracle(x.double().reshape((n,) + dims + (c,)), gamma.double(), beta.double(), g, mode).reshape(x.shape)
    assert rel(y, want) <= 1e-12


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SMALL_GN, ids=str)
def test_backward_formula_equals_autograd(shape, mode, relu):
    n, dims, c, g = shape
    x, dy, gamma, beta = N.gn_inputs(shape, mode, seams=False)      # (outliers in a unit of 2 elements: fp64 itself cancels to 1e-8)
    st = N.gn_stats_ref(x, g, mode, abi_eps=False)
    ref = N.gn_bwd_ref(x, dy, gamma, beta, st['mean'], st['rstd'], g, mode, relu)
    dx, dgamma, dbeta = N.gn_bwd_autograd(x, dy, gamma, beta, g, mode, relu)
    assert not ref['undecided'].any()
    # dx against the size of the terms it is the difference of (a unit of 2 elements normalises to +-1: its dx cancels to 0)
    scale = max(float(dx.abs().max()), float(ref['b_dx'].max()) / (N.K_EW * N.EPS32))
    assert float((ref['dx'] - dx).abs().max()) <= 1e-10 * scale
    assert rel(ref['dgamma'], dgamma) <= 1e-10 and rel(ref['dbeta'], dbeta) <= 1e-10


@pytest.mark.parametrize('conv', [True, False])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', N.GATE_SHAPES, ids=str)
def test_gate_references_equal_autograd(shape, mode, conv):
    """resnet.py:121-137 as tests/test_kernels_gpu.py::test_se_gate_epilogue_fwd_bwd restates it"""
    n, dims, f, r, g = shape
    v = N.nvox(dims)
    p = N.gate_inputs(shape)
    rd = p['res'].double().requires_grad_(True)
    w1d, w2d, wspd = [p[k].double().requires_grad_(True) for k in ('w1', 'w2', 'wsp')]
    gap = rd.mean(dim=1)
    hh = torch.relu(gap @ w1d)
    ch = torch.sigmoid(hh @ w2d)
    sp = torch.sigmoid(rd @ wspd)
    out = rd * (sp.unsqueeze(-1) + ch.reshape(n, 1, f))
    st = N.gn_stats_ref(p['c2'], g, mode, abi_eps=False)
    if conv:
        c5 = p['c2'].double().reshape((n,) + dims + (f,))
        out = out + torch.relu(N.group_norm_oracle(c5, p['gamma'].double(), p['beta'].double(), g, mode)).reshape(n, v, f)
    out.backward(p['dout'].double())
    h_r, _, ch_r, _ = N.se_mlp_ref(gap.detach(), p['w1'], p['w2'])
    assert rel(h_r, hh.detach()) <= 1e-12 and rel(ch_r, ch.detach()) <= 1e-12
    sp_r, _, out_r, _ = N.epilogue_ref(p['res'], p['c2'] if conv else None, p['wsp'], ch.detach(), p['gamma'], p['beta'], st['mean'],
                                       st['rstd'], g, mode)
    assert rel(sp_r, sp.detach()) <= 1e-12 and rel(out_r, out.detach()) <= 1e-12
    b = N.se_bwd_ref(p['dout'], p['res'], sp.detach(), gap.detach(), hh.detach(), ch.detach(), p['w1'], p['w2'], p['wsp'])
    for name, want in (('dres', rd.grad), ('dw1', w1d.grad), ('dw2', w2d.grad), ('dwsp', wspd.grad)):
        assert rel(b[name], want) <= 1e-10, name


# ---------------------------------------------------------------------------------------------------------------
# the restatements against the references
# ---------------------------------------------------------------------------------------------------------------
def _gn_case(shape, mode, kind, relu, accumulate=False):
    n, dims, c, g = shape
    x, dy, gamma, beta = N.gn_inputs(shape, mode, kind)
    tag = '%s mode %d %s relu %d' % (shape, mode, kind, relu)
    st = N.gn_stats_ref(x, g, mode)
    mean, rstd = N.gn_stats_f32(x, g, mode)
    held('gn_stats mean ' + tag, mean, st['mean'], st['b_mean'])
    held('gn_stats rstd ' + tag, rstd, st['rstd'], st['b_rstd'])
    y, b_y, _ = N.gn_apply_ref(x, gamma, beta, mean, rstd, g, mode, relu)
    held('gn_apply general ' + tag, N.gn_apply_f32(x, gamma, beta, mean, rstd, g, mode, relu, False), y, b_y)
    held('gn_apply streaming ' + tag, N.gn_apply_f32(x, gamma, beta, mean, rstd, g, mode, relu, True), y, b_y)
    old = (torch.randn(c, generator=N._gen(3)), torch.randn(c, generator=N._gen(4))) if accumulate else (None, None)
    ref = N.gn_bwd_ref(x, dy, gamma, beta, mean, rstd, g, mode, relu, *old)
    dx, dgamma, dbeta = N.gn_bwd_f32(x, dy, gamma, beta, mean, rstd, g, mode, relu, *old)
    r = N.ratio_either(dx, ref['dx'], ref['dx_alt'], ref['b_dx'])
    print('%-58s %.3f (limit 0.25)' % ('gn_bwd dx ' + tag, r))
    assert r <= 0.25
    held('gn_bwd dgamma ' + tag, dgamma, ref['dgamma'], ref['b_dgamma'], 1.0 if accumulate else 0.25)
    held('gn_bwd dbeta ' + tag, dbeta, ref['dbeta'], ref['b_dbeta'], 1.0)
    share = float(ref['undecided'].double().mean())
    assert share <= N.UNDECIDED_CAP, 'undecided share %.2e: take another seed' % share


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SMALL_GN, ids=str)
def test_groupnorm_restatements(shape, mode, relu):
    _gn_case(shape, mode, 'wide', relu)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [N.GN_SHAPE_RAGGED, N.GN_SHAPE_STREAM], ids=str)
def test_groupnorm_restatements_offset_input_and_accumulation(shape, mode):
    _gn_case(shape, mode, 'offset', 1, accumulate=True)


@pytest.mark.parametrize('shape,mode', [(N.GN_SHAPE_BLOCK_CAP, N.SLAB), (N.GN_SHAPE_BLOCK_CAP, N.CHANNEL), (N.GN_SHAPE_GENERIC_CAP, N.SLAB),
                                        (N.GN_SHAPE_GENERIC_CAP, N.CHANNEL), (N.GN_SHAPE_VECTOR_CAP, N.CHANNEL)], ids=str)
def test_groupnorm_restatements_large(shape, mode):
    _gn_case(shape, mode, 'wide', 1)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', N.GN_CONSTANT_SHAPES, ids=str)
def test_constant_volume_reaches_the_clamp(shape, mode):
    """the fp32 square of the constant lies below its exact square, so the kernel's E[x^2] - mean^2 is negative where the squares are
    rounded (the vectorised slab kernel) and 0 elsewhere: clamped, rstd within its bound of 1 / sqrt(eps)"""
    n, dims, c, g = shape
    x, dy, gamma, beta = N.gn_inputs(shape, mode, 'constant')
    xx = torch.tensor(N.CONSTANT_VALUE, dtype=torch.float32)
    assert float((xx * xx).double()) < float(xx.double() ** 2)
    st = N.gn_stats_ref(x, g, mode)
    assert float((st['rstd'] - 1.0 / N.f32(N.GN_EPS) ** 0.5).abs().max()) <= 1e-9
    mean, rstd = N.gn_stats_f32(x, g, mode)
    assert torch.isfinite(rstd).all()
    held('constant mean', mean, st['mean'], st['b_mean'])
    held('constant rstd', rstd, st['rstd'], st['b_rstd'])
    dx, _, _ = N.gn_bwd_f32(x, dy, gamma, beta, mean, rstd, g, mode, 1)
    assert torch.isfinite(dx).all()


@pytest.mark.parametrize('n,f,r', N.MLP_SHAPES + [(s[0], s[2], s[3]) for s in N.GATE_SHAPES], ids=str)
def test_se_mlp_restatement(n, f, r):
    gen = N._gen(77)
    gap = torch.randn((n, f), generator=gen)
    w1 = torch.randn((f, r), generator=gen) / f ** 0.5
    w2 = torch.randn((r, f), generator=gen) * 2.0 / r ** 0.5
    h_r, b_h, ch_r, b_ch = N.se_mlp_ref(gap, w1, w2)
    h, ch = N.se_mlp_f32(gap, w1, w2)
    chain = max(f // max(256 // r, 1), r)
    held('se_mlp h (%d,%d,%d)' % (n, f, r), h, h_r, b_h, N.LONG_CHAIN_HOST_LIMIT if chain >= 24 else 0.25)
    held('se_mlp ch (%d,%d,%d)' % (n, f, r), ch, ch_r, b_ch, N.LONG_CHAIN_HOST_LIMIT if chain >= 24 else 0.25)


def _gate_case(shape, mode, conv, accumulate):
    n, dims, f, r, g = shape
    p = N.gate_inputs(shape)
    tag = '%s mode %d conv %d' % (shape, mode, conv)
    mean, rstd = N.gn_stats_f32(p['c2'], g, mode)
    gap = p['res'].double().mean(1).float()
    h, ch = N.se_mlp_f32(gap, p['w1'], p['w2'])
    c2 = p['c2'] if conv else None
    sp_r, b_sp, out_r, b_out = N.epilogue_ref(p['res'], c2, p['wsp'], ch, p['gamma'], p['beta'], mean, rstd, g, mode)
    sp, out = N.epilogue_f32(p['res'], c2, p['wsp'], ch, p['gamma'], p['beta'], mean, rstd, g, mode)
    held('epilogue sp ' + tag, sp, sp_r, b_sp)
    held('epilogue out ' + tag, out, out_r, b_out)
    q = N.gate_inputs(shape, seams='gate')
    old = dict((k, torch.randn(q[w].shape, generator=N._gen(5))) for k, w in (('dw1', 'w1'), ('dw2', 'w2'), ('dwsp', 'wsp'))) if accumulate else None
    args = (q['dout'], q['res'], q['sp_in'], q['gap_in'], h, ch, q['w1'], q['w2'], q['wsp'])
    ref = N.se_bwd_ref(*args, old=old)
    got = N.se_bwd_f32(*args, old=old)
    for k in N.GATE_OUTPUTS:
        held('se_bwd %s %s' % (k, tag), got[k], ref[k], ref['b_' + k], 1.0 if accumulate and k in ('dw1', 'dw2', 'dwsp') else 0.25)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', N.GATE_SHAPES, ids=str)
def test_gate_restatements(shape, mode):
    _gate_case(shape, mode, True, False)
    _gate_case(shape, mode, False, True)


def test_gate_restatements_large():
    _gate_case(N.GATE_SHAPE_CAP, N.SLAB, True, False)


# ---------------------------------------------------------------------------------------------------------------
# seams: every seam item is worth 8 bounds of some output (on the reference alone)
# ---------------------------------------------------------------------------------------------------------------
def _gn_seam_case(shape, mode, kind='wide'):
    n, dims, c, g = shape
    v = N.nvox(dims)
    x, dy, gamma, beta = N.gn_inputs(shape, mode, kind)
    items = N.gn_seams(n, v, c, g, mode)
    unit = N._unit_of(n, v, c, g, mode)
    st = N.gn_stats_ref(x, g, mode)
    xd = x.double().reshape(-1)
    u0 = unit[items[:, 0]]
    same = (unit[items] == u0[:, None]).double()
    dS, dQ = (xd[items] * same).sum(1), (xd[items] ** 2 * same).sum(1)
    m0, r0 = N.gn_stats_from_sums(st['s'], st['q'], st['L'], st['eps'])
    worst = float('inf')
    for sign in (-1.0, 1.0):      # dropped, counted twice
        m1, r1 = N.gn_stats_from_sums(st['s'][u0] + sign * dS, st['q'][u0] + sign * dQ, st['L'], st['eps'])
        moved = torch.maximum((m1 - m0[u0]).abs() / st['b_mean'][u0], (r1 - r0[u0]).abs() / st['b_rstd'][u0])
        worst = min(worst, float(moved.min()))
    print('%-58s stats: the weakest seam item moves an output by %.1f bounds' % ('%s mode %d' % (shape, mode), worst))
    assert worst >= 8.0
    mean, rstd = N.gn_stats_f32(x, g, mode)
    for relu in (0, 1):
        ref = N.gn_bwd_ref(x, dy, gamma, beta, mean, rstd, g, mode, relu)
        _, idx = N.gn_index(v, c, g, mode)
        de = ref['de'].reshape(-1)[items].abs()
        moved = (de / ref['b_dbeta'][idx[items % (v * c)]]).max(1).values
        if relu and 4 * items.numel() > x.numel():      # (all seams: x is random there, the mask removes some items; see norm_ref)
            moved = moved[de.max(1).values > 0]
        print('%-58s bwd relu %d: %.3g bounds' % ('', relu, float(moved.min())))
        assert float(moved.min()) >= 8.0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SMALL_GN + [N.GN_SHAPE_BLOCK_CAP], ids=str)
def test_groupnorm_seam_items_are_worth_eight_bounds(shape, mode):
    _gn_seam_case(shape, mode)


def test_groupnorm_seam_items_large_and_offset():
    _gn_seam_case(N.GN_SHAPE_VECTOR_CAP, N.CHANNEL)
    _gn_seam_case(N.GN_SHAPE_GENERIC_CAP, N.SLAB)
    _gn_seam_case(N.GN_SHAPE_RAGGED, N.SLAB, 'offset')
    _gn_seam_case(N.GN_SHAPE_RAGGED, N.CHANNEL, 'offset')


def _gate_seam_moves(q, ref, h, ch, sv, n, v, f):
    """per seam voxel: the largest move, in bounds, of dw2 (through Pch) or dwsp when the voxel is dropped or counted twice"""
    d, r = q['dout'].double().reshape(n * v, f)[sv], q['res'].double().reshape(n * v, f)[sv]
    nn = sv // v
    sg = (ch.double() * (1.0 - ch.double()))[nn]
    dw2 = h.double()[nn][:, :, None].abs() * (sg * d * r).abs()[:, None, :] / ref['b_dw2'][None]
    dwsp = (ref['ds'].reshape(-1)[sv][:, None] * r).abs() / ref['b_dwsp'][None]
    return torch.maximum(dw2.flatten(1).max(1).values, dwsp.max(1).values)


@pytest.mark.parametrize('shape', N.GATE_SHAPES + [N.GATE_SHAPE_CAP], ids=str)
def test_gate_seam_voxels_are_worth_eight_bounds(shape):
    n, dims, f, r, g = shape
    v = N.nvox(dims)
    q = N.gate_inputs(shape, seams='gate')
    h, ch = N.se_mlp_f32(q['gap_in'], q['w1'], q['w2'])
    ref = N.se_bwd_ref(q['dout'], q['res'], q['sp_in'], q['gap_in'], h, ch, q['w1'], q['w2'], q['wsp'])
    moved = _gate_seam_moves(q, ref, h, ch, q['seam_voxels'], n, v, f)
    print('%-58s %.3g bounds' % (shape, float(moved.min())))
    assert float(moved.min()) >= 8.0


@pytest.mark.parametrize('shape', N.BLOCK_SHAPES + [N.BLOCK_SHAPE_CAP], ids=str)
def test_fused_seam_voxels_are_worth_eight_bounds(shape):
    n, dims, f, r, g = shape
    v = N.nvox(dims)
    q = N.gate_inputs(shape, seams='blk')
    h, ch = N.se_mlp_f32(q['gap_in'], q['w1'], q['w2'])
    ref = N.se_bwd_ref(q['dout'], q['res'], q['sp_in'], q['gap_in'], h, ch, q['w1'], q['w2'], q['wsp'])
    moved = _gate_seam_moves(q, ref, h, ch, q['seam_voxels'], n, v, f)
    assert float(moved.min()) >= 8.0
    mean, rstd = N.gn_stats_f32(q['c2'], g, N.SLAB)
    gn = N.gn_bwd_ref(q['c2'], q['dout'], q['gamma'], q['beta'], mean, rstd, g, N.SLAB, 1)
    items = N.gn_seams(n, v, f, g, N.SLAB)
    _, idx = N.gn_index(v, f, g, N.SLAB)
    m2 = (gn['de'].reshape(-1)[items].abs() / gn['b_dbeta'][idx[items % (v * f)]]).max(1).values
    print('%-58s gate %.3g, GroupNorm %.3g bounds' % (shape, float(moved.min()), float(m2.min())))
    assert float(m2.min()) >= 8.0
    share = float(gn['undecided'].double().mean())
    assert share <= N.UNDECIDED_CAP, 'undecided share %.2e: take another seed' % share


# ---------------------------------------------------------------------------------------------------------------
# control: the bounds tell a dropped element and a wrong divisor from rounding (restatements only)
# ---------------------------------------------------------------------------------------------------------------
def test_control_dropped_element_and_wrong_divisor_fail_the_gpu_side_bound():
    shape, mode = N.GN_SHAPE_RAGGED, N.SLAB
    n, dims, c, g = shape
    x, dy, gamma, beta = N.gn_inputs(shape, mode)
    L = N.gn_geom(n, N.nvox(dims), c, g, mode)['L']
    last = 1 * L + L - 1      # the last element of the ragged second span of unit (0, 1)
    st = N.gn_stats_ref(x, g, mode)
    mean, rstd = N.gn_stats_f32(x, g, mode)
    m_bad, r_bad = N.gn_stats_f32(x, g, mode, drop=last)
    a = max(N.ratio(m_bad, st['mean'], st['b_mean']), N.ratio(r_bad, st['rstd'], st['b_rstd']))
    ref = N.gn_bwd_ref(x, dy, gamma, beta, mean, rstd, g, mode, 1)
    _, dg_bad, db_bad = N.gn_bwd_f32(x, dy, gamma, beta, mean, rstd, g, mode, 1, drop=last)
    b = max(N.ratio(dg_bad, ref['dgamma'], ref['b_dgamma']), N.ratio(db_bad, ref['dbeta'], ref['b_dbeta']))
    dx_bad, _, _ = N.gn_bwd_f32(x, dy, gamma, beta, mean, rstd, g, mode, 1, c1_count=L - 1)
    c = N.ratio_either(dx_bad, ref['dx'], ref['dx_alt'], ref['b_dx'])
    print('control: dropped last element of a ragged span: statistics %.3g, dgamma / dbeta %.3g of the bound; L - 1 in c1: dx %.3g' % (a, b, c))
    assert a > 8.0 and b > 8.0 and c > 8.0


# ---------------------------------------------------------------------------------------------------------------
# argument statuses: every call returns before its first HIP call (read from the sources); nothing is launched.
# bts_se_mlp_fwd and bts_se_bwd have no status for an operand off a 16-byte boundary (the gate's parameter views are not promised
# aligned, include/bts_hip.h); bts_se_bwd's BTS_ERR_ALIGN is its workspace's.
# ---------------------------------------------------------------------------------------------------------------
A = 4096        # a "pointer": 16-byte aligned, never dereferenced
OFF4 = 4100     # 4 bytes off a 16-byte boundary
BIG = 1 << 30
SH, AL, UN, WS = -1, -2, -3, -4


def _stats(x=A, ws=A, wsb=BIG, n=1, v=8, c=16, g=8, mode=0):
    return (x, A, A, ws, wsb, n, v, c, g, mode, 1e-5, None)


def _apply(x=A, y=A, n=1, v=8, c=16, ldy=16, g=8, mode=0):
    return (x, y, A, A, A, A, n, v, c, ldy, g, mode, 1, None)


def _gnbwd(x=A, dy=A, dx=A, ws=A, wsb=BIG, n=1, v=8, c=16, lddy=16, g=8, mode=0):
    return (x, dy, dx, A, A, A, A, A, A, ws, wsb, n, v, c, lddy, g, mode, 1, 0, None)


def _epi(res=A, c2=A, out=A, n=1, v=8, f=16, ldo=16, g=8):
    return (res, c2, out, A, A, A, A, A, A, A, n, v, f, ldo, g, 0, None)


def _sebwd(ws=A, wsb=BIG, n=1, v=8, f=16, r=2, lddo=16):
    return (A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, ws, wsb, n, v, f, r, lddo, 0, None)


def _blk(dout=A, lddo=16, res=A, c2=A, ws=A, wsb=BIG, n=1, v=512, f=16, r=2, g=8):
    return (dout, lddo, res, c2, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, ws, wsb, n, v, f, r, g, 0, 0, None)


STATUS_CASES = [
    ('bts_gn_workspace G does not divide C', 'bts_gn_workspace', (1, 8, 12, 5, 0), -1),
    ('bts_gn_workspace C < G', 'bts_gn_workspace', (1, 8, 4, 8, 1), -1),
    ('bts_gn_workspace N = 0', 'bts_gn_workspace', (0, 8, 16, 8, 0), -1),
    ('bts_gn_bwd_workspace G does not divide C', 'bts_gn_bwd_workspace', (1, 8, 12, 5, 0), -1),
    ('bts_gn_bwd_workspace V = 0', 'bts_gn_bwd_workspace', (1, 0, 16, 8, 1), -1),
    ('bts_gn_stats G does not divide C', 'bts_gn_stats', _stats(c=12, g=5), SH),
    ('bts_gn_stats G = 0', 'bts_gn_stats', _stats(g=0), SH),
    ('bts_gn_stats short workspace', 'bts_gn_stats', _stats(wsb=8), WS),
    ('bts_gn_stats NULL workspace', 'bts_gn_stats', _stats(ws=None), WS),
    ('bts_gn_stats NULL workspace, generic shape', 'bts_gn_stats', _stats(ws=None, c=12, g=3), WS),
    ('bts_gn_stats x 4 bytes off', 'bts_gn_stats', _stats(x=OFF4), AL),
    ('bts_gn_stats x 4 bytes off, channel mode', 'bts_gn_stats', _stats(x=OFF4, mode=1), AL),
    ('bts_gn_apply C < G', 'bts_gn_apply', _apply(c=4, ldy=4), SH),
    ('bts_gn_apply ldy < C', 'bts_gn_apply', _apply(ldy=12), AL),
    ('bts_gn_apply ldy < C, generic shape', 'bts_gn_apply', _apply(c=12, g=3, ldy=10), AL),
    ('bts_gn_apply x 4 bytes off', 'bts_gn_apply', _apply(x=OFF4), AL),
    ('bts_gn_apply y 4 bytes off', 'bts_gn_apply', _apply(y=OFF4, ldy=32), AL),
    ('bts_gn_bwd G does not divide C', 'bts_gn_bwd', _gnbwd(c=12, g=5, lddy=12), SH),
    ('bts_gn_bwd lddy < C', 'bts_gn_bwd', _gnbwd(lddy=12), AL),
    ('bts_gn_bwd lddy < C, generic shape', 'bts_gn_bwd', _gnbwd(c=12, g=3, lddy=8), AL),
    ('bts_gn_bwd short workspace', 'bts_gn_bwd', _gnbwd(wsb=64), WS),
    ('bts_gn_bwd short workspace, generic shape', 'bts_gn_bwd', _gnbwd(wsb=8, c=12, g=3, lddy=12), WS),
    ('bts_gn_bwd short workspace, lddy % 4 != 0', 'bts_gn_bwd', _gnbwd(wsb=8, lddy=18), WS),
    ('bts_gn_bwd NULL workspace', 'bts_gn_bwd', _gnbwd(ws=None), WS),
    ('bts_gn_bwd dy 4 bytes off', 'bts_gn_bwd', _gnbwd(dy=OFF4, lddy=32), AL),
    ('bts_gn_bwd dx 4 bytes off', 'bts_gn_bwd', _gnbwd(dx=OFF4), AL),
    ('bts_gn_bwd x 4 bytes off, channel mode', 'bts_gn_bwd', _gnbwd(x=OFF4, mode=1), AL),
    ('bts_se_mlp_fwd N = 0', 'bts_se_mlp_fwd', (A, A, A, A, A, 0, 16, 2, None), SH),
    ('bts_se_mlp_fwd R = 0', 'bts_se_mlp_fwd', (A, A, A, A, A, 1, 16, 0, None), SH),
    ('bts_block_epilogue_fwd F = 2', 'bts_block_epilogue_fwd', _epi(f=2, ldo=4, g=2), SH),
    ('bts_block_epilogue_fwd F = 12', 'bts_block_epilogue_fwd', _epi(f=12, ldo=12, g=3), SH),
    ('bts_block_epilogue_fwd F = 512', 'bts_block_epilogue_fwd', _epi(f=512, ldo=512), SH),
    ('bts_block_epilogue_fwd ldo % 4 != 0', 'bts_block_epilogue_fwd', _epi(ldo=18), SH),
    ('bts_block_epilogue_fwd ldo < F', 'bts_block_epilogue_fwd', _epi(ldo=12), SH),
    ('bts_block_epilogue_fwd G does not divide F', 'bts_block_epilogue_fwd', _epi(g=3), SH),
    ('bts_block_epilogue_fwd res 4 bytes off', 'bts_block_epilogue_fwd', _epi(res=OFF4), AL),
    ('bts_block_epilogue_fwd out 4 bytes off', 'bts_block_epilogue_fwd', _epi(out=OFF4, ldo=32), AL),
    ('bts_block_epilogue_fwd c2 4 bytes off', 'bts_block_epilogue_fwd', _epi(c2=OFF4), AL),
    ('bts_se_bwd_workspace F = 2', 'bts_se_bwd_workspace', (1, 8, 2, 1), -1),
    ('bts_se_bwd_workspace F = 12', 'bts_se_bwd_workspace', (1, 8, 12, 1), -1),
    ('bts_se_bwd_workspace N = 0', 'bts_se_bwd_workspace', (0, 8, 16, 2), -1),
    ('bts_se_bwd F = 12', 'bts_se_bwd', _sebwd(f=12, lddo=12), SH),
    ('bts_se_bwd F = 2', 'bts_se_bwd', _sebwd(f=2, lddo=4), SH),
    ('bts_se_bwd F = 512', 'bts_se_bwd', _sebwd(f=512, lddo=512), SH),
    ('bts_se_bwd R = 0', 'bts_se_bwd', _sebwd(r=0), SH),
    ('bts_se_bwd lddo < F', 'bts_se_bwd', _sebwd(lddo=12), SH),
    ('bts_se_bwd lddo % 4 != 0', 'bts_se_bwd', _sebwd(lddo=18), SH),
    ('bts_se_bwd short workspace', 'bts_se_bwd', _sebwd(wsb=64), WS),
    ('bts_se_bwd NULL workspace', 'bts_se_bwd', _sebwd(ws=None), WS),
    ('bts_se_bwd workspace 8 bytes off', 'bts_se_bwd', _sebwd(ws=A + 8), AL),
    ('bts_block_bwd_workspace unit not whole chunks', 'bts_block_bwd_workspace', (1, 64, 8, 2, 4), -1),
    ('bts_block_bwd_workspace F = 24', 'bts_block_bwd_workspace', (1, 512, 24, 2, 8), -1),
    ('bts_block_bwd unit not whole chunks', 'bts_block_bwd', _blk(v=64, f=8, lddo=8, g=4), UN),
    ('bts_block_bwd lddo < F', 'bts_block_bwd', _blk(lddo=12), AL),
    ('bts_block_bwd lddo % 4 != 0', 'bts_block_bwd', _blk(lddo=18), AL),
    ('bts_block_bwd dout 4 bytes off', 'bts_block_bwd', _blk(dout=OFF4, lddo=32), AL),
    ('bts_block_bwd res 4 bytes off', 'bts_block_bwd', _blk(res=OFF4), AL),
    ('bts_block_bwd c2 4 bytes off', 'bts_block_bwd', _blk(c2=OFF4), AL),
    ('bts_block_bwd NULL workspace', 'bts_block_bwd', _blk(ws=None), WS),
    ('bts_block_bwd short workspace', 'bts_block_bwd', _blk(wsb=64), WS),
    ('bts_block_bwd workspace 8 bytes off', 'bts_block_bwd', _blk(ws=A + 8), WS),
]


@pytest.mark.parametrize('what,name,args,status', STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_argument_status(what, name, args, status):
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    assert len(args) == len(L.protos[name][1]), 'argument list does not match the header'
    assert getattr(L, '_' + name)(*args) == status


def test_workspace_queries_of_good_shapes_are_positive():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    for n, dims, c, g in N.GN_SHAPES + [N.GN_SHAPE_BLOCK_CAP, N.GN_SHAPE_GENERIC_CAP, N.GN_SHAPE_VECTOR_CAP]:
        for mode in MODES:
            assert 0 < L._bts_gn_workspace(n, N.nvox(dims), c, g, mode) < L._bts_gn_bwd_workspace(n, N.nvox(dims), c, g, mode)
    for n, dims, f, r, g in N.GATE_SHAPES + [N.GATE_SHAPE_CAP]:
        assert L._bts_se_bwd_workspace(n, N.nvox(dims), f, r) > 0


def test_block_bwd_workspace_declines_exactly_where_block_bwd_takes_says_no(monkeypatch):
    """the query, ops.block_bwd_takes (on dense, aligned tensors: only the tiling is left to decide) and norm_ref's restatement of
    blk_bwd_plan agree on a grid of shapes around every condition of the plan"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    from bts_amd._lib import lib
    monkeypatch.setattr(ops._core, '_check', lambda *a, **k: None)      # (the tensors are never touched: CPU stand-ins; patched where the wrappers look it up)
    L = lib()
    took = 0
    for n in (1, 3):
        for dims in ((1, 1, 1), (1, 2, 2), (2, 2, 2), (4, 4, 4), (4, 6, 8), (6, 10, 14), (8, 8, 16)):
            for f in (2, 4, 8, 12, 16, 24, 64, 128, 256, 512):
                for g in (1, 3, 4, 8):
                    for r in (0, 1, 4):
                        v = N.nvox(dims)
                        ws = L._bts_block_bwd_workspace(n, v, f, r, g)
                        plan = N.block_bwd_plan(n, v, f, r, g)
                        assert (ws >= 0) == plan, (n, dims, f, r, g, ws)
                        assert ws == -1 or ws > 0
                        t = torch.empty((n,) + dims + (f,))
                        assert ops.block_bwd_takes(t, r, g, t, t) == plan, (n, dims, f, r, g)
                        took += plan
    assert took > 20
    for shape in N.BLOCK_SHAPES + [N.BLOCK_SHAPE_CAP]:
        n, dims, f, r, g = shape
        assert N.block_bwd_plan(n, N.nvox(dims), f, r, g), shape


def test_listed_shapes_reach_the_paths_they_name():
    """the geometry each shape is listed for, from the restated host arithmetic"""
    G = N.gn_geom
    assert G(1, 1, 16, 8, 0)['generic'] and G(2, 16, 12, 3, 0)['generic'] and G(2, 64, 2, 2, 1)['generic']
    q = G(3, 840, 16, 8, N.SLAB)
    assert not q['generic'] and (q['L'], q['span'], q['B']) == (1680, 1024, 2)
    q = G(3, 840, 16, 8, N.CHANNEL)
    assert (q['unit'], q['span'], q['B']) == (13440, 1024, 14) and 13440 - 13 * 1024 == 128
    assert [N.gn_stream_cpb(*s) for s in ((1, 192, 128, 8, 0), (1, 768, 64, 8, 0), (1, 512, 64, 8, 0), (1, 4096, 16, 8, 0))] == [1, 2, 4, 8]
    q = G(1, 32 * 32 * 48, 64, 8, N.SLAB)
    assert (q['span'], q['B']) == (2048, 192) and 2048 // 8 == 256
    q = G(1, 8, 1024, 2, N.SLAB)
    assert not q['generic'] and q['cg'] == 512
    assert 48 ** 3 * 20 > 8192 * 256 and G(1, 48 ** 3, 20, 4, 0)['generic']
    assert 64 * 64 * 66 * 32 > 8192 * 1024 and N.gn_stream_cpb(1, 64 * 64 * 66, 32, 8, N.CHANNEL) == 0
    assert N.gn_stream_cpb(3, 840, 16, 8, N.SLAB, ld=32) == 0 and N.gn_stream_cpb(1, 768, 64, 8, N.SLAB, ld=80) == 2
    assert N.gn_stream_cpb(1, 768, 64, 8, N.SLAB, ld=66) == 0
    assert N.se_bwd_blocks(840, 3, 16) == (14, 64, 64) and 840 - 13 * 64 == 8
    assert N.se_bwd_blocks(1, 1, 4)[2] == 256 and N.se_bwd_blocks(12, 1, 256)[2] == 4
    assert 64 * 64 * 66 > 8192 * (256 // (32 // 4)) and 64 * 64 * 66 * (32 // 4) > 8192 * 256
