"""-m gpu: the fp32 weight gradient runs the kernel its host-side choice names.  One call per kernel of bts_conv3d_bwd_weight, at the
smallest shape that reaches it: bts_conv3d_bwd_weight_kernel is asked first, the one weight-gradient launch the profiler records must be
the kernel it named (the finalize launch and the swapped form's column sum are not profiled), and dW -- db too where the kind has one --
meets the fp64 oracle, once plain and once accumulated onto itself.

Tolerance: the contraction bound of test_wgw3_gpu.py, |err| <= 8 * eps32 * sum|a_i b_i| + 1e-7; the bound tensor is the oracle on
|x|, |dy|."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_kernels_gpu import _profiled, check_contraction, dev, ref_conv, rnd, wshape  # noqa: E402

K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
SWITCHES = ('BTS_WGW', 'BTS_K1W')
# name: kind, (D, H, W) of x, Cin, Cout, db asked for, channels of the slab x is cut from one channel in (0: x dense), switches, kernel
CASES = {
    'wgw': (K3S1, (2, 4, 16), 32, 32, True, 0, {}, 24),
    'fixed sweep behind BTS_WGW=0': (K3S1, (2, 4, 16), 32, 32, True, 0, {'BTS_WGW': '0'}, 109),
    'stride-2 sweep': (K3S2, (2, 8, 16), 32, 32, True, 0, {}, 110),
    'stride-2 sweep, transposed': (K3S2T, (1, 4, 8), 32, 32, False, 0, {}, 110),
    'LDS-DMA staging, ragged 3x3x3': (K3S1, (3, 5, 18), 32, 32, True, 0, {}, 104),
    'LDS-DMA staging, small 1x1x1': (K1, (4, 8, 16), 32, 32, True, 0, {}, 104),
    'register staging, two input channels': (K3S1, (3, 5, 18), 2, 32, True, 0, {}, 100),
    'register staging, swapped form and its column sum': (K3S1, (3, 5, 18), 32, 2, True, 0, {}, 100),
    'register staging, x off its 16-byte boundary': (K3S1, (2, 4, 16), 32, 32, True, 40, {}, 100),
    'k1w at its threshold': (K1, (32, 32, 32), 32, 32, True, 0, {}, 26),
    'k1w, odd extents and channel groups': (K1, (33, 31, 35), 64, 24, True, 0, {}, 26),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_weight_gradient_runs_the_kernel_the_query_names(monkeypatch, case):
    from bts_amd import ops
    kind, (d, h, w), cin, cout, want_db, slab, env, want = CASES[case]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x = rnd((1, d, h, w, cin), 71)
    wd = torch.zeros(wshape(kind, cin, cout), dtype=torch.float64, requires_grad=True)
    bd = torch.zeros((cout,), dtype=torch.float64, requires_grad=True)
    y = ref_conv(kind, x.double(), wd, bd)
    dy = rnd(tuple(y.shape), 72)
    y.backward(dy.double())
    wa = torch.zeros_like(wd, requires_grad=True)
    ref_conv(kind, x.double().abs(), wa, None).backward(dy.double().abs())
    dw_ref, dw_bound, db_ref, db_bound = wd.grad, wa.grad, bd.grad, dy.double().abs().sum(dim=(0, 1, 2, 3))
    if slab:
        wide = torch.zeros((1, d, h, w, slab), device=dev())
        xg = wide[..., 1:1 + cin]
        xg.copy_(x)
        assert xg.data_ptr() % 16 == 4
    else:
        xg = x.to(dev())
    dyg = dy.to(dev())
    sym = ops.conv_bwd_weight_kernel(kind, xg, dyg)
    assert sym == want, (case, sym)
    assert (ops.conv_bwd_weight_form(kind, xg, dyg) == 3) == (sym == 24)
    dw = torch.empty(wshape(kind, cin, cout), device=dev())
    db = torch.empty((cout,), device=dev()) if want_db else None
    _, names = _profiled(lambda: ops.conv_bwd_weight(kind, xg, dyg, dw, db))
    assert names == [ops.kernel_symbol(sym)], (case, names, sym)
    check_contraction(dw, dw_ref, dw_bound, case + ': dW')
    if want_db:
        check_contraction(db, db_ref, db_bound, case + ': db')
    ops.conv_bwd_weight(kind, xg, dyg, dw, db, accumulate=True)
    check_contraction(dw, 2 * dw_ref, 2 * dw_bound, case + ': dW accumulated')
    if want_db:
        check_contraction(db, 2 * db_ref, 2 * db_bound, case + ': db accumulated')
