"""-m gpu: every config and form of the tiled fp32 conv kernel (igemm_kernel) against the fp64 oracle.  One call per row of
tests/tiled_cases.py: bts_conv3d_kernel is asked first, the one conv launch the profiler records must be the kernel it named (the split-K
reduce and the GroupNorm finalize are not profiled), and the result meets the oracle.  tests/test_tiled_configs_host.py keeps the table
complete: every (direction, kind, form, config) a layer of the model runs on the tiled kernel has a row here.

Tolerance: the contraction bound of test_kernels_gpu.py, |err| <= 8 * eps32 * sum|a_i b_i| + 1e-7 with the bound tensor from the oracle
on absolute values, the same for every row.  An accumulating call adds onto a seeded tensor d0: one more term, |d0|, in the
bound.  The one row with the sigmoid is held after the activation: the sigmoid's slope is at most 1/4, so the contraction's share is a
quarter of the bound above, and the activation itself gets the element-wise tolerance 1e-6 + 1e-5 |ref| of SURVEY 8c.  GroupNorm
statistics: the bounds of test_conv_with_fused_groupnorm_statistics (rtol 2e-5, atol 2e-5) against fp64 moments of the fp64 conv.

Every row prints `tiled-row | name | symbol | worst error as a multiple of its tolerance` (pytest -s shows it)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as R  # noqa: E402
from test_kernels_gpu import EPS32, _named, _profiled, _route_env, check_close, check_contraction, dev, ref_conv, rnd, wshape  # noqa: E402
import tiled_cases as T  # noqa: E402

SENTINEL = -7.5          # what the other channels of a slab hold
UNWRITTEN = 1.0e30       # what a dense output holds before the call: an element the kernel skips is far outside every tolerance


def held(r, got, ref, bound, what):
    """check_contraction, after printing the worst error as a multiple of the tolerance; a NaN compares false there, so finiteness first"""
    assert bool(torch.isfinite(got).all()), '%s: %s holds a non-finite value' % (r.name, what)
    err = (got.double().cpu() - ref).abs()
    worst = float((err / (8 * EPS32 * bound + 1e-7)).max())
    print('tiled-row | %s | %s | sym %d | %.3f of the bound' % (r.name, what, r.sym, worst))
    check_contraction(got, ref, bound, '%s: %s' % (r.name, what))
    return worst


def read_operand(r, t):
    """t on the device: dense, or channels [1, 1 + C) of a slab of C + 3 channels (4 bytes off a 16-byte boundary, odd rows)"""
    if not r.xslab:
        return t.to(dev())
    wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), SENTINEL, device=dev())
    view = wide[..., 1:1 + t.shape[-1]]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def written_operand(r, shape, before):
    """(the tensor the call writes, its slab or None): dense, or channels [4, 4 + C) of a slab of C + 8 channels; it holds `before` (the
    tensor an accumulating call adds onto) or UNWRITTEN"""
    if r.yslab:
        slab = torch.full(tuple(shape[:-1]) + (shape[-1] + 8,), SENTINEL, device=dev())
        out = slab[..., 4:4 + shape[-1]]
    else:
        slab, out = None, torch.empty(shape, device=dev())
    if before is None:
        out.fill_(UNWRITTEN)
    else:
        out.copy_(before)
    return out, slab


def slab_kept(r, slab, c):
    if slab is not None:
        assert bool((slab[..., :4] == SENTINEL).all()) and bool((slab[..., 4 + c:] == SENTINEL).all()), r.name + ': the slab\'s other channels changed'


def moments(ref, n, g):
    flat = ref.reshape(n, g, -1)
    return flat.mean(dim=2).reshape(-1), (1.0 / torch.sqrt(flat.var(dim=2, unbiased=False) + 1e-5)).reshape(-1)


def forward(r, L, ops, want):
    d, h, w = r.dims
    x, wt = rnd((r.n, d, h, w, r.cin), 101), rnd(wshape(r.kind, r.cin, r.cout), 102, 0.2)
    b = rnd((r.cout,), 103) if r.bias else None
    xd, xa = x.double(), x.double().abs()
    ref = ref_conv(r.kind, xd, wt.double(), None if b is None else b.double())
    bound = ref_conv(r.kind, xa, wt.double().abs(), None if b is None else b.double().abs())
    xg = read_operand(r, x)
    bg = None if b is None else b.to(dev())
    wp = ops.conv_pack(r.kind, ops.ROLE_FWD, wt.to(dev()), r.cin, r.cout)
    if r.second == T.Y2:
        w1, b1 = rnd((1, 1, 1, r.cin, r.cout), 104, 0.3), rnd((r.cout,), 105)
        wp1 = ops.conv_pack(ops.K1, ops.ROLE_FWD, w1.to(dev()), r.cin, r.cout)
        assert L._bts_conv3d_fwd_can_fuse(r.n, d, h, w, r.cin, r.cout) == (r.sym != T.UNSUPPORTED)
        if r.sym == T.UNSUPPORTED:
            c1, res = torch.empty(tuple(ref.shape), device=dev()), torch.empty(tuple(ref.shape), device=dev())
            status = L._bts_conv3d_fwd_fused2(ops._p(xg), ops._p(wp), ops._p(bg), ops._p(c1), ops._p(wp1), ops._p(b1.to(dev())), ops._p(res),
                                              r.n, d, h, w, r.cin, ops.ld_of(xg), r.cout, r.cout, r.cout, ops._stream())
            assert status == T.UNSUPPORTED, status
            assert ops.conv_fwd_fused2(xg, wp, bg, wp1, b1.to(dev()), r.cout) is None      # (the caller then runs the two convs apart)
            return
        (c1, res), names = _profiled(lambda: ops.conv_fwd_fused2(xg, wp, bg, wp1, b1.to(dev()), r.cout))
        assert names == [want], (r.name, names, want)
        held(r, c1, ref, bound, 'y')
        held(r, res, R.conv3d(xd, w1.double(), b1.double()), R.conv3d(xa, w1.double().abs(), b1.double().abs()), 'y2')
        return
    if r.groups:
        (y, mean, rstd), names = _profiled(lambda: ops.conv_fwd_gn(r.kind, xg, wp, bg, r.cout, r.groups, 1e-5))
        assert names == [want], (r.name, names, want)
        held(r, y, ref, bound, 'y')
        mean_r, rstd_r = moments(ref, r.n, r.groups)
        check_close(mean, mean_r, r.name + ': GroupNorm mean', rtol=2e-5, atol=2e-5)
        check_close(rstd, rstd_r, r.name + ': GroupNorm rstd', rtol=2e-5, atol=2e-5)
        return
    out, slab = written_operand(r, tuple(ref.shape), None)
    _, names = _profiled(lambda: ops.conv_fwd(r.kind, xg, wp, bg, r.cout, out=out, sigmoid=r.sigmoid))
    assert names == [want], (r.name, names, want)
    if r.sigmoid:
        assert bool(torch.isfinite(out).all())
        sref = torch.sigmoid(ref)
        err = (out.double().cpu() - sref).abs()
        tol = 0.25 * (8 * EPS32 * bound + 1e-7) + 1e-6 + 1e-5 * sref
        print('tiled-row | %s | sigmoid(y) | sym %d | %.3f of the tolerance' % (r.name, r.sym, float((err / tol).max())))
        assert not bool((err > tol).any()), '%s: %d elements out of tolerance, max err %.3e' % (r.name, int((err > tol).sum()), float(err.max()))
    else:
        held(r, out, ref, bound, 'y')
    slab_kept(r, slab, r.cout)


def data_gradient(r, L, ops, want):
    d, h, w = r.dims
    wt = rnd(wshape(r.kind, r.cin, r.cout), 102, 0.2)
    x0 = torch.zeros((r.n, d, h, w, r.cin), dtype=torch.float64)      # (the conv is linear: its gradient does not depend on x)
    xd, xa = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    y = ref_conv(r.kind, xd, wt.double(), None)
    dy = rnd(tuple(y.shape), 106)
    loss, loss_a = (y * dy.double()).sum(), (ref_conv(r.kind, xa, wt.double().abs(), None) * dy.double().abs()).sum()
    if r.second == T.X2:
        w1, dy2 = rnd((1, 1, 1, r.cin, r.cout), 104, 0.3), rnd(tuple(y.shape), 107)
        loss = loss + (R.conv3d(xd, w1.double(), None) * dy2.double()).sum()
        loss_a = loss_a + (R.conv3d(xa, w1.double().abs(), None) * dy2.double().abs()).sum()
    loss.backward()
    loss_a.backward()
    ref, bound = xd.grad, xa.grad
    d0 = rnd(tuple(x0.shape), 108) if r.accumulate else None
    if r.accumulate:
        ref, bound = ref + d0.double(), bound + d0.double().abs()
    dyg = read_operand(r, dy)
    wpb = ops.conv_pack(r.kind, ops.ROLE_BWD, wt.to(dev()), r.cin, r.cout)
    dx, slab = written_operand(r, tuple(x0.shape), d0)
    if r.second == T.X2:
        wpb1 = ops.conv_pack(ops.K1, ops.ROLE_BWD, w1.to(dev()), r.cin, r.cout)
        dy2g = dy2.to(dev())
        _, names = _profiled(lambda: ops.conv_bwd_data_pair(dyg, wpb, dy2g, wpb1, dx, r.accumulate))
    else:
        _, names = _profiled(lambda: ops.conv_bwd_data(r.kind, dyg, wpb, dx, r.accumulate))
    assert names == [want], (r.name, names, want)
    held(r, dx, ref, bound, 'dx')
    slab_kept(r, slab, r.cin)


@pytest.mark.parametrize('name', [r.name for r in T.ROWS])
def test_tiled_kernel_row_runs_the_named_config_and_meets_the_oracle(monkeypatch, name):
    from bts_amd import ops
    from bts_amd._lib import lib
    r = T.by_name()[name]
    L = lib()
    _route_env(monkeypatch, r.env)
    sym = T.named(L, r)
    assert sym == r.sym, (r.name, sym)
    want = None if sym < 0 else ops.kernel_symbol(sym)
    assert want is None or want.startswith('igemm_kernel'), want
    if not (r.xslab or r.yslab or r.sigmoid or r.accumulate or r.groups or sym < 0):      # (_named describes dense operands and no flags)
        assert _named(r.direction, r.kind, r.n, r.dims, r.cin, r.cout, r.second) == want
    assert (T.workspace(L, r) > 0) == r.splitk, (r.name, T.workspace(L, r))
    (forward if r.direction == T.FWD else data_gradient)(r, L, ops, want)
