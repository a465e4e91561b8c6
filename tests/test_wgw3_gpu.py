"""-m gpu: the three-axis Winograd form F(2x2x2, 3x3x3) of the stride-1 3x3x3 weight gradient (wgw_kernel in csrc/conv_wgw.hip)
against the fp64 oracle, through bts_conv3d_bwd_weight.  Which form took a call is asked of the host
query bts_conv3d_bwd_weight_form: 3 three-axis | 0 direct (BTS_WGW=0).  The two-axis form (2) it replaced lost at every layer shape
and left with its switch, so no call can report it.

Tolerance: the contraction bound of test_wgw_gpu.py, |err| <= 8 * eps32 * sum|a_i b_i| + 1e-7; the bound tensor is the oracle on
|x|, |dy|.  Unit impulses must come out exactly: every transform matrix entry is 0, +-1 or +-1/2."""
import contextlib
import itertools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as R  # noqa: E402

EPS32 = 2.0 ** -24
DIRECT, THREE_AXIS = 0, 3


def dev():
    return torch.device('cuda:0')


def rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32)


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    tol = 8 * EPS32 * bound + 1e-7
    bad = err > tol
    worst = float((err / tol).max())
    print('%s: max err / tol %.3f' % (what, worst))
    assert not bad.any(), '%s: %d/%d out of tolerance, max err %.3e (tol there %.3e), max|ref| %.3e' % (
        what, int(bad.sum()), bad.numel(), float(err.max()), float(tol.flatten()[err.argmax()]), float(ref.abs().max()))


def oracle(x, dy):
    """-> dW, its bound (the oracle on |x|, |dy|), db, its bound; all fp64 on the CPU"""
    cin, cout = x.shape[-1], dy.shape[-1]
    wd = torch.zeros((3, 3, 3, cin, cout), dtype=torch.float64, requires_grad=True)
    bd = torch.zeros((cout,), dtype=torch.float64, requires_grad=True)
    (R.conv3d(x.double(), wd, bd) * dy.double()).sum().backward()
    wa = torch.zeros((3, 3, 3, cin, cout), dtype=torch.float64, requires_grad=True)
    (R.conv3d(x.double().abs(), wa, None) * dy.double().abs()).sum().backward()
    return wd.grad, wa.grad, bd.grad, dy.double().abs().sum(dim=(0, 1, 2, 3))


def forms_of(xg, dyg):
    """the host query's answer as called and under BTS_WGW=0"""
    from bts_amd import ops
    a = ops.conv_bwd_weight_form(ops.K3S1, xg, dyg)
    with env(BTS_WGW='0'):
        c = ops.conv_bwd_weight_form(ops.K3S1, xg, dyg)
    return a, c


def ran_wgw(fn):
    from bts_amd import ops
    ops.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    names = [r[0] for r in ops.profile_records()]
    ops.profile_enable(False)
    return 'wgw_kernel' in names


def test_wgw3_exact_tap_placement():
    """x and dy are unit impulses: dW has a single 1 at the tap that joins the two voxels (none if that tap leaves the volume) and
    must equal the oracle exactly.  All 27 offsets, for dy voxels at each of the 8 positions inside a 2x2x2 patch, at the eight
    corners of the volume (one per position: even sizes) and in the interior across sub-tile borders."""
    from bts_amd import ops
    d, h, w, c = 4, 8, 32, 32
    xg = torch.zeros((1, d, h, w, c), device=dev())
    dyg = torch.zeros((1, d, h, w, c), device=dev())
    dw = torch.empty((3, 3, 3, c, c), device=dev())
    assert forms_of(xg, dyg) == (THREE_AXIS, DIRECT)
    x1 = torch.zeros((1, d, h, w, 1), dtype=torch.float64)
    dy1 = torch.zeros((1, d, h, w, 1), dtype=torch.float64)
    case = 0
    for par in itertools.product((0, 1), repeat=3):
        corner = tuple(p * (n - 1) for p, n in zip(par, (d, h, w)))
        inner = (2 - par[0], 4 - par[1], 16 - par[2])   # same parities, on either side of the sub-tile borders at z = 2, y = 4, x = 16
        for v in (corner, inner):
            assert tuple(i % 2 for i in v) == par
            for off in itertools.product((-1, 0, 1), repeat=3):
                u = tuple(a + b for a, b in zip(v, off))
                inside = all(0 <= a < n for a, n in zip(u, (d, h, w)))
                uc = tuple(min(max(a, 0), n - 1) for a, n in zip(u, (d, h, w)))   # outside: some voxel next to it instead
                ci, co = (7 * case + 3) % c, (11 * case + 5) % c
                case += 1
                x1[(0,) + uc + (0,)] = 1.0
                dy1[(0,) + v + (0,)] = 1.0
                wd = torch.zeros((3, 3, 3, 1, 1), dtype=torch.float64, requires_grad=True)
                (R.conv3d(x1, wd, None) * dy1).sum().backward()   # the oracle on the two live channels; all others are zero
                x1[(0,) + uc + (0,)] = 0.0
                dy1[(0,) + v + (0,)] = 0.0
                if inside:
                    assert float(wd.grad.sum()) == 1.0 and float(wd.grad[off[0] + 1, off[1] + 1, off[2] + 1, 0, 0]) == 1.0
                ref = torch.zeros((3, 3, 3, c, c), dtype=torch.float32)
                ref[:, :, :, ci, co] = wd.grad[:, :, :, 0, 0].float()
                xg[(0,) + uc + (ci,)] = 1.0
                dyg[(0,) + v + (co,)] = 1.0
                ops.conv_bwd_weight(ops.K3S1, xg, dyg, dw, None)
                xg[(0,) + uc + (ci,)] = 0.0
                dyg[(0,) + v + (co,)] = 0.0
                assert torch.equal(dw.cpu(), ref), 'dy at %s, x at %s (offset %s), channels %d -> %d: %s' % (
                    v, uc, off, ci, co, (dw.cpu() - ref).nonzero().tolist()[:8])
    assert case == 8 * 2 * 27


# one sub-tile with every patch on a border | N = 2, two P groups and three Q groups | several sub-tiles on every axis
SMALL = [(1, (2, 4, 16), 32, 32), (2, (2, 4, 16), 64, 96), (1, (6, 12, 48), 32, 64)]


@pytest.mark.parametrize('n,dims,cin,cout', SMALL)
def test_wgw3_smallest_shapes_against_oracle(n, dims, cin, cout):
    from bts_amd import ops
    d, h, w = dims
    x, dy = rnd((n, d, h, w, cin), 1), rnd((n, d, h, w, cout), 2)
    wd, wa, bd, bb = oracle(x, dy)
    xg, dyg = x.to(dev()), dy.to(dev())
    assert forms_of(xg, dyg) == (THREE_AXIS, DIRECT)
    dw = torch.empty((3, 3, 3, cin, cout), device=dev())
    db = torch.empty((cout,), device=dev())
    assert ran_wgw(lambda: ops.conv_bwd_weight(ops.K3S1, xg, dyg, dw, db))
    check(dw, wd, wa, 'wgw3 dW')
    check(db, bd, bb, 'wgw3 db')
    ops.conv_bwd_weight(ops.K3S1, xg, dyg, dw, db, accumulate=True)
    check(dw, 2 * wd, 2 * wa, 'wgw3 dW accumulate')
    check(db, 2 * bd, 2 * bb, 'wgw3 db accumulate')


def test_wgw3_several_subtiles_per_workgroup_and_short_last_one():
    """(26, 20, 80): 13 x 5 x 5 = 325 sub-tiles, planned as 163 workgroups of 2 with the last of 1 (the workspace size tells: 27 x 1024
    floats + 32 doubles per workgroup) -- both LDS buffers in turn and the clipped tail"""
    from bts_amd import ops
    from bts_amd._lib import lib
    n, (d, h, w), cin, cout = 1, (26, 20, 80), 32, 32
    nb = lib().query('bts_conv3d_bwd_weight_workspace', ops.K3S1, n, d, h, w, cin, cout)
    nsp = nb // (27 * 1024 * 4 + 32 * 8)
    nsub = (d // 2) * (h // 4) * (w // 16)
    assert nsub == 325 and 1 < nsp < nsub and nsub % nsp != 0 and -(-nsub // nsp) >= 2, (nsub, nsp)
    x, dy = rnd((n, d, h, w, cin), 3), rnd((n, d, h, w, cout), 4)
    wd, wa, bd, bb = oracle(x, dy)
    xg, dyg = x.to(dev()), dy.to(dev())
    assert forms_of(xg, dyg) == (THREE_AXIS, DIRECT)
    dw = torch.empty((3, 3, 3, cin, cout), device=dev())
    db = torch.empty((cout,), device=dev())
    assert ran_wgw(lambda: ops.conv_bwd_weight(ops.K3S1, xg, dyg, dw, db))
    check(dw, wd, wa, 'wgw3 dW, 2 sub-tiles per workgroup')
    check(db, bd, bb, 'wgw3 db, 2 sub-tiles per workgroup')


def test_wgw3_slab_views_and_folded_duplicate_slice():
    """the arguments of test_wgw_gpu.py's test of the same name: x and dy as channel slices of wider slabs (ld > C) and the encoder's
    duplicated input slice, scattered back to both copies by the shared finalize kernel"""
    from bts_amd import ops
    n, d, h, w, f, j = 1, 4, 8, 16, 32, 2
    cin_slab, cin_ref, cout = j * f, (j + 1) * f, 32
    slab = rnd((n, d, h, w, cin_slab + 32), 8)
    dslab = rnd((n, d, h, w, cout + 16), 9)
    xs = slab[..., :cin_slab]
    dyd = dslab[..., 16:]
    wd, wa, _, _ = oracle(torch.cat([xs[..., (j - 1) * f:], xs], dim=-1), dyd)
    sg, dg = slab.to(dev()), dslab.to(dev())
    xg, dyg = sg[..., :cin_slab], dg[..., 16:]
    assert forms_of(xg, dyg) == (THREE_AXIS, DIRECT)
    dw = torch.empty((3, 3, 3, cin_ref, cout), device=dev())
    assert ran_wgw(lambda: ops.conv_bwd_weight(ops.K3S1, xg, dyg, dw, None, (j - 1) * f, f))
    check(dw, wd, wa, 'wgw3 folded, strided dW')


def test_wgw3_is_bitwise_deterministic_and_the_forms_agree():
    """(16, 16, 64), 32 -> 32: two calls give the same bits; the three-axis and the direct form each lie within the bound of the
    oracle"""
    from bts_amd import ops
    x, dy = rnd((1, 16, 16, 64, 32), 21), rnd((1, 16, 16, 64, 32), 22)
    wd, wa, bd, bb = oracle(x, dy)
    xg, dyg = x.to(dev()), dy.to(dev())
    assert forms_of(xg, dyg) == (THREE_AXIS, DIRECT)
    a, b = (torch.empty((3, 3, 3, 32, 32), device=dev()) for _ in range(2))
    da, dbb = (torch.empty((32,), device=dev()) for _ in range(2))
    ops.conv_bwd_weight(ops.K3S1, xg, dyg, a, da)
    ops.conv_bwd_weight(ops.K3S1, xg, dyg, b, dbb)
    assert torch.equal(a, b) and torch.equal(da, dbb)
    check(a, wd, wa, 'three-axis dW')
    check(da, bd, bb, 'three-axis db')
    with env(BTS_WGW='0'):
        assert not ran_wgw(lambda: ops.conv_bwd_weight(ops.K3S1, xg, dyg, b, dbb))
    check(b, wd, wa, 'direct dW')
    check(dbb, bd, bb, 'direct db')
