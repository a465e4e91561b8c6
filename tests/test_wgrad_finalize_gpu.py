"""-m gpu: the fp32 weight gradient's finalize pass (conv_wgfin.hip) where the other weight-gradient tests do not reach it: the lane
kernel wgrad_finalize_kernel (more than 16 partials) with packed (tap, channel) rows, with a folded slab and in the transposed
layout, and the swapped form with a fold on its Q axis in both kernels.  dW -- db too where the case asks for one -- meets the
fp64 oracle, once plain and once accumulated onto itself; a folded case's oracle is the duplicated formulation of
test_kernels_gpu.test_conv_folded_duplicate_slice.

The finalize launch is not profiled, so each case proves which finalize kernel it reaches from the workspace query: for one
(P, Q) channel-tile pair the workspace is nsp * (ntiles * 4096 + 256) + 384 bytes, plus bts_colsum_workspace for the swapped form,
and nsp <= 16 goes to the flat kernel.  A later change of the K-split fails the case instead of moving its coverage.

Tolerance: the contraction bound of test_wgrad_plan_gpu.py, |err| <= 8 * eps32 * sum|a_i b_i| + 1e-7; the bound tensor is the
oracle on |x|, |dy|."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_kernels_gpu import check_contraction, dev, ref_conv, rnd, wshape  # noqa: E402

K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
DUP_START, DUP_SHIFT = 16, 16
# name: kind, (D, H, W) of x, slab Cin, Cout, folded (the reference has Cin + DUP_SHIFT input channels), db asked for, swapped form,
#       row-tiles per partial, partials, finalize kernel
CASES = {
    'fold on the P axis, 27 tiles': (K3S1, (4, 16, 48), 32, 32, True, False, False, 27, 24, 'lane'),
    'packed rows, lane': (K3S1, (4, 16, 48), 2, 32, False, True, False, 2, 24, 'lane'),
    'packed rows, flat': (K3S1, (3, 5, 18), 2, 32, False, True, False, 2, 8, 'flat'),
    'swapped form, fold on the Q axis, flat': (K3S1, (8, 8, 8), 32, 4, True, True, True, 4, 4, 'flat'),
    'swapped form, fold on the Q axis, lane': (K3S1, (4, 16, 48), 32, 4, True, True, True, 4, 24, 'lane'),
    'transposed layout': (K3S2T, (4, 8, 24), 32, 32, False, False, False, 27, 24, 'lane'),
    '1x1x1, fold': (K1, (8, 16, 48), 32, 32, True, True, False, 1, 32, 'lane'),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_weight_gradient_finalize(monkeypatch, case):
    from bts_amd import ops
    from bts_amd._lib import lib
    kind, (d, h, w), cin, cout, folded, want_db, swapped, ntiles, nsp, fin = CASES[case]
    for k in ('BTS_WGW', 'BTS_K1W'):
        monkeypatch.delenv(k, raising=False)
    # the partial count, from the workspace query
    nb = lib().query('bts_conv3d_bwd_weight_workspace', kind, 1, d, h, w, cin, cout)
    if swapped:
        nb -= lib().query('bts_colsum_workspace', 1, d * h * w, cout)
    per = ntiles * 4096 + 256
    assert (nb - 384) % per == 0 and (nb - 384) // per == nsp, (case, nb)
    assert (nsp <= 16) == (fin == 'flat')

    x = rnd((1, d, h, w, cin), 81)
    xd = x.double()
    if folded:      # the duplicated formulation: reference channels [slab[DUP_START:], slab]
        xd = torch.cat([xd[..., DUP_START:], xd], dim=-1)
    cin_ref = xd.shape[-1]
    wd = torch.zeros(wshape(kind, cin_ref, cout), dtype=torch.float64, requires_grad=True)
    bd = torch.zeros((cout,), dtype=torch.float64, requires_grad=True)
    y = ref_conv(kind, xd, wd, bd)
    dy = rnd(tuple(y.shape), 82)
    y.backward(dy.double())
    wa = torch.zeros_like(wd, requires_grad=True)
    ref_conv(kind, xd.abs(), wa, None).backward(dy.double().abs())
    dw_ref, dw_bound, db_ref, db_bound = wd.grad, wa.grad, bd.grad, dy.double().abs().sum(dim=(0, 1, 2, 3))

    xg, dyg = x.to(dev()), dy.to(dev())
    dw = torch.empty(wshape(kind, cin_ref, cout), device=dev())
    db = torch.empty((cout,), device=dev()) if want_db else None
    fold = (DUP_START, DUP_SHIFT) if folded else (0, 0)
    ops.conv_bwd_weight(kind, xg, dyg, dw, db, *fold)
    check_contraction(dw, dw_ref, dw_bound, case + ': dW')
    if want_db:
        check_contraction(db, db_ref, db_bound, case + ': db')
    ops.conv_bwd_weight(kind, xg, dyg, dw, db, *fold, accumulate=True)
    check_contraction(dw, 2 * dw_ref, 2 * dw_bound, case + ': dW accumulated')
    if want_db:
        check_contraction(db, 2 * db_ref, 2 * db_bound, case + ': db accumulated')
