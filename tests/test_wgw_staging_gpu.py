"""-m gpu: the staging of wgw_kernel (csrc/conv_wgw.hip) at the smallest shapes where it can go wrong.  A thread stages the four
z rows of one (y row, x, channel quad) column of the P halo tile, each z row through a descriptor of its own, and writes the four
xi_z planes d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3; every group of requests goes out two steps before its LDS write, groups 0 and
1 of a sub-tile in the last two steps of the sub-tile before.  So: columns on every face (a plane must not come from the
neighbouring sample), exactly two sub-tiles along each axis in turn (the deeper fetch crosses a sub-tile border), three sub-tiles
per workgroup with a short last one (requests two steps deep behind the workgroup's end, both LDS buffers more than once), a
sample boundary inside a workgroup's run, channel slices of wider slabs, and exact unit impulses on either side of a sub-tile's
z border.

Tolerance: the contraction bound of test_wgw3_gpu.py, |err| <= 8 * eps32 * sum|a_i b_i| + 1e-7, the bound tensor being the fp64
oracle on |x|, |dy|.  Unit impulses must come out exactly."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as R  # noqa: E402

EPS32 = 2.0 ** -24
THREE_AXIS = 3


def dev():
    return torch.device('cuda:0')


def rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32)


def check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    tol = 8 * EPS32 * bound + 1e-7
    bad = err > tol
    print('%s: max err / tol %.3f' % (what, float((err / tol).max())))
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


def ran_wgw(fn):
    from bts_amd import ops
    ops.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    names = [r[0] for r in ops.profile_records()]
    ops.profile_enable(False)
    return 'wgw_kernel' in names


def run_case(n, dims, cin, cout, seed, what):
    from bts_amd import ops
    d, h, w = dims
    x, dy = rnd((n, d, h, w, cin), seed), rnd((n, d, h, w, cout), seed + 1)
    wd, wa, bd, bb = oracle(x, dy)
    xg, dyg = x.to(dev()), dy.to(dev())
    assert ops.conv_bwd_weight_form(ops.K3S1, xg, dyg) == THREE_AXIS
    dw = torch.empty((3, 3, 3, cin, cout), device=dev())
    db = torch.empty((cout,), device=dev())
    assert ran_wgw(lambda: ops.conv_bwd_weight(ops.K3S1, xg, dyg, dw, db))
    check(dw, wd, wa, what + ' dW')
    check(db, bd, bb, what + ' db')


@pytest.mark.parametrize('n', [1, 2])
def test_staging_one_subtile_every_column_on_a_face(n):
    """(2, 4, 16): z rows 0 and 3 of every column lie outside the sample -- with N = 2 inside the neighbouring one, which must not
    be read"""
    run_case(n, (2, 4, 16), 32, 32, 31 + n, 'one sub-tile, N = %d' % n)


@pytest.mark.parametrize('dims', [(4, 4, 16), (2, 8, 16), (2, 4, 32)])
def test_staging_two_subtiles_along_one_axis(dims):
    run_case(1, dims, 32, 32, 41 + dims[0] + dims[1], 'two sub-tiles %s' % (dims,))


def test_staging_three_subtiles_per_workgroup_and_short_last_one():
    """(28, 20, 160): 14 x 5 x 10 = 700 sub-tiles, planned as 234 workgroups of 3 with the last of 1 (the workspace size tells: 27 x
    1024 floats + 32 doubles per workgroup)"""
    from bts_amd import ops
    from bts_amd._lib import lib
    n, (d, h, w), cin, cout = 1, (28, 20, 160), 32, 32
    nb = lib().query('bts_conv3d_bwd_weight_workspace', ops.K3S1, n, d, h, w, cin, cout)
    nsp = nb // (27 * 1024 * 4 + 32 * 8)
    nsub = (d // 2) * (h // 4) * (w // 16)
    assert nsub == 700 and nsp == 234 and -(-nsub // nsp) == 3 and nsub % 3 != 0, (nsub, nsp)
    run_case(n, (d, h, w), cin, cout, 51, '3 sub-tiles per workgroup')


def test_staging_sample_boundary_inside_a_run_two_p_groups_three_q_groups():
    run_case(2, (4, 8, 32), 64, 96, 61, 'N = 2, 64 -> 96')


def test_staging_slab_views():
    """the arguments of test_wgw3_gpu.py's slab test at (4, 8, 32): x and dy as channel slices of wider slabs (ld > C) and the
    encoder's duplicated input slice, scattered back to both copies by the shared finalize kernel"""
    from bts_amd import ops
    n, d, h, w, f, j = 1, 4, 8, 32, 32, 2
    cin_slab, cin_ref, cout = j * f, (j + 1) * f, 32
    slab = rnd((n, d, h, w, cin_slab + 32), 8)
    dslab = rnd((n, d, h, w, cout + 16), 9)
    xs = slab[..., :cin_slab]
    dyd = dslab[..., 16:]
    wd, wa, _, _ = oracle(torch.cat([xs[..., (j - 1) * f:], xs], dim=-1), dyd)
    sg, dg = slab.to(dev()), dslab.to(dev())
    xg, dyg = sg[..., :cin_slab], dg[..., 16:]
    assert ops.conv_bwd_weight_form(ops.K3S1, xg, dyg) == THREE_AXIS
    dw = torch.empty((3, 3, 3, cin_ref, cout), device=dev())
    assert ran_wgw(lambda: ops.conv_bwd_weight(ops.K3S1, xg, dyg, dw, None, (j - 1) * f, f))
    check(dw, wd, wa, 'slab views dW')


def test_staging_two_calls_are_bit_identical():
    from bts_amd import ops
    x, dy = rnd((2, 4, 8, 32, 32), 71), rnd((2, 4, 8, 32, 32), 72)
    xg, dyg = x.to(dev()), dy.to(dev())
    a, b = (torch.empty((3, 3, 3, 32, 32), device=dev()) for _ in range(2))
    da, db = (torch.empty((32,), device=dev()) for _ in range(2))
    assert ran_wgw(lambda: ops.conv_bwd_weight(ops.K3S1, xg, dyg, a, da))
    ops.conv_bwd_weight(ops.K3S1, xg, dyg, b, db)
    assert torch.equal(a, b) and torch.equal(da, db)


def test_staging_unit_impulses_across_the_z_border_are_exact():
    """(4, 8, 32): dy is a unit impulse at z = 0, 1 | 2, 3 (first plane, either side of the sub-tile border at z = 2, last plane), at
    the y and x sub-tile borders; x a unit impulse at each of the 27 neighbours.  dW has a single 1 at the tap that joins the two
    voxels (none if that tap leaves the volume) and must equal the oracle exactly: a z plane formed from the wrong rows, or with a
    row of the neighbouring sub-tile, moves or doubles it."""
    from bts_amd import ops
    d, h, w, c = 4, 8, 32, 32
    xg = torch.zeros((1, d, h, w, c), device=dev())
    dyg = torch.zeros((1, d, h, w, c), device=dev())
    dw = torch.empty((3, 3, 3, c, c), device=dev())
    assert ops.conv_bwd_weight_form(ops.K3S1, xg, dyg) == THREE_AXIS
    x1 = torch.zeros((1, d, h, w, 1), dtype=torch.float64)
    dy1 = torch.zeros((1, d, h, w, 1), dtype=torch.float64)
    case = 0
    for z in range(d):
        v = (z, 4 - (z & 1), 16 - (z >> 1))
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
    assert case == 4 * 27
