"""-m gpu: the data-gradient pair of a ResNet block, dx (+)= conv3x3x3^T(dy) + conv1x1x1^T(dy2), with the Winograd F(2x2x2,3x3x3)
kernel forming the 1x1x1 term in its own output side (csrc/conv_wino3.hip, w3_kernel<true>): one launch instead of w3_kernel + the
streaming 1x1x1 kernel.  BTS_WINO_MIN_WGS=1 and BTS_IGEMM_K1S_MIN=1 let the small shapes used here take the form; every case asks
bts_conv3d_bwd_data_pair_launches what the call takes and asserts through the profiler that exactly that ran: ['w3_kernel'] where the
query says 1, two entries where it says 2.

The pair fuses only where no kernel of the 3x3x3 gradient may split the contraction (its workspace query answers 0).  At 2 x 4x8x32
64 -> 48 and 1 x 8x8x32 32 -> 32 the query does not answer 0, so these two shapes run as two calls and are checked as such; the
properties they were chosen for are covered in the one-launch form by 2 x 4x8x32 24 -> 48 (two cout blocks, the second half full,
N = 2), by 1 x 20x36x72 32 -> 16 under BTS_W3_T=4 (chains of four items per workgroup, the last chain of an XCD one item long) and by
1 x 20x36x72 40 -> 16 (five k-groups of dy2: the first fragment buffer is requested a second time, its second k-group masked).  Both
fragment buffers requested and consumed a second time -- what the 64-channel level of the model runs -- is 1 x 32x32x96 64 -> 16, the
smallest shape found at which no kernel of the 3x3x3 gradient splits 64 channels; it also carries unit impulses in all eight k-groups.

Tolerance: that of tests/test_wino_gpu.py, |err| <= 32 * eps32 * sum|a_i b_i| + 1e-7 with the sum over both terms (and |old dx| when
accumulating).  K2 -> C below: dy and dy2 have K2 channels, dx has C."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from guard_alloc import FILL, install  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

EPS32 = 2.0 ** -24
ENV = dict(BTS_WINO_MIN_WGS='1', BTS_IGEMM_K1S_MIN='1')
SWITCHES = ('BTS_WINO', 'BTS_W3', 'BTS_W3_T', 'BTS_WINO_MIN_WGS', 'BTS_IGEMM_DSC_MIN', 'BTS_IGEMM_C2_MIN', 'BTS_IGEMM_K1S_MIN',
            'BTS_IGEMM_UPM_MIN', 'BTS_IGEMM_NOGNFUSE', 'BTS_IGEMM_NOPAIR')


def dev():
    return torch.device('cuda:0')


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


_CASE = {}


def case_data(n, dims, k2, c):
    """inputs, fp64 reference and bound of one shape: computed once, shared, never changed"""
    key = (n, dims, k2, c)
    if key not in _CASE:
        d, h, w = dims
        w3, w1 = rnd((3, 3, 3, c, k2), 11, 0.2), rnd((1, 1, 1, c, k2), 12, 0.3)
        dy, dy2, old = rnd((n, d, h, w, k2), 13), rnd((n, d, h, w, k2), 14), rnd((n, d, h, w, c), 15)
        x = torch.zeros((n, d, h, w, c), dtype=torch.float64, requires_grad=True)
        ((R.conv3d(x, w3.double(), None) * dy.double()).sum() + (R.conv3d(x, w1.double(), None) * dy2.double()).sum()).backward()
        xa = torch.zeros((n, d, h, w, c), dtype=torch.float64, requires_grad=True)
        ((R.conv3d(xa, w3.double().abs(), None) * dy.double().abs()).sum() +
         (R.conv3d(xa, w1.double().abs(), None) * dy2.double().abs()).sum()).backward()
        _CASE[key] = dict(w3=w3, w1=w1, dy=dy, dy2=dy2, old=old, ref=x.grad.detach(), bound=xa.grad.detach())
    return _CASE[key]


def tol_of(bound):
    return 32 * EPS32 * bound + 1e-7


def check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    tol = tol_of(bound)
    ratio = float((err / tol).max())
    print('%s: worst error / bound = %.4f' % (what, ratio))
    bad = err > tol
    assert not bad.any(), '%s: %d/%d elements out of tolerance, worst error / bound %.3f' % (what, int(bad.sum()), bad.numel(), ratio)
    return ratio


def aligned_bits(dy, dx, dy2):
    return (dy.data_ptr() % 16 == 0) | (dx.data_ptr() % 16 == 0) << 1 | (dy2.data_ptr() % 16 == 0) << 2 | 8


def run_pair(dy, w3, dy2, w1, dx, accumulate, want=None):
    """one pair call under the profiler -> the launch record; asserted against the host query (and against `want` launches when given)"""
    from bts_amd import ops
    from bts_amd._lib import lib
    n, d, h, w, c = dx.shape
    k2 = dy.shape[4]
    wpb3 = ops.conv_pack(ops.K3S1, ops.ROLE_BWD, w3.to(dev()), c, k2)
    wpb1 = ops.conv_pack(ops.K1, ops.ROLE_BWD, w1.to(dev()), c, k2)
    torch.cuda.synchronize()
    said = lib()._bts_conv3d_bwd_data_pair_launches(n, d, h, w, c, ops.ld_of(dx), k2, ops.ld_of(dy), ops.ld_of(dy2), 2 if accumulate else 0,
                                                    aligned_bits(dy, dx, dy2), -1)
    assert said in (1, 2), said
    if want is not None:
        assert said == want, (said, want)
    ops.profile_enable(True)
    try:
        ops.conv_bwd_data_pair(dy, wpb3, dy2, wpb1, dx, accumulate)
        torch.cuda.synchronize()
    finally:
        ops.profile_enable(False)
    names = [r[0] for r in ops.profile_records()]
    if said == 1:
        assert names == ['w3_kernel'], names
    else:
        assert len(names) == 2, names
    return names


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)


# N, (D, H, W), K2, C, launches the query must claim, BTS_W3_T
SHAPES = [
    (1, (4, 4, 12), 8, 16, 1, None),        # one tile, three quarters of it in x
    (1, (5, 6, 14), 24, 24, 1, None),       # ragged in every axis, three k-groups: half of the second fragment buffer unused
    (2, (4, 8, 32), 64, 48, 2, None),       # (the 3x3x3 gradient may split the contraction: two calls)
    (2, (4, 8, 32), 24, 48, 1, None),       # two cout blocks, the second half full, N = 2
    (1, (8, 8, 32), 32, 32, 2, '3'),        # (as above: two calls)
    (1, (20, 36, 72), 32, 16, 1, '4'),      # 29 items per XCD in chains of 4: a last chain of one; the k-group count of level 0
    (1, (20, 36, 72), 40, 16, 1, None),     # five k-groups: the first fragment buffer requested a second time, half of it used
    (1, (32, 32, 96), 64, 16, 1, None),     # eight k-groups, the k-group count of level 1: both buffers requested and used a second time
]


@pytest.mark.parametrize('n,dims,k2,c,want,chain', SHAPES, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
def test_pair_meets_the_oracle(monkeypatch, n, dims, k2, c, want, chain, accumulate):
    if chain:
        monkeypatch.setenv('BTS_W3_T', chain)
    q = case_data(n, dims, k2, c)
    dx = q['old'].to(dev()).clone() if accumulate else torch.full((n,) + dims + (c,), float('nan'), device=dev())
    run_pair(q['dy'].to(dev()), q['w3'], q['dy2'].to(dev()), q['w1'], dx, accumulate, want)
    ref, bound = (q['ref'] + q['old'].double(), q['bound'] + q['old'].double().abs()) if accumulate else (q['ref'], q['bound'])
    check(dx, ref, bound, 'pair %s %d->%d' % (dims, k2, c))


@pytest.mark.parametrize('flip', [0, 4], ids=['half0', 'half1'])
@pytest.mark.parametrize('dims,k2,c', [((4, 4, 32), 16, 48), ((32, 32, 96), 64, 16)], ids=['2kg', '8kg'])
def test_unit_impulses_land_exactly(flip, dims, k2, c):
    """dy = 0 and dy2 a unit impulse at chosen (voxel, channel) pairs: dx at such a voxel is that channel's row of w1 bit for bit, and
    0 everywhere else.  1 x 4x4x32 is two tiles of 32 patches; 16 -> 48 is two k-groups and two cout blocks.  The voxels: all 8
    positions of the first and of the last patch of both tiles; the channels walk both halves of both k-groups (`flip` swaps halves).
    1 x 32x32x96 64 -> 16: the same voxels (first two tiles of the volume), the channels walk all eight k-groups, those of the second
    request of either fragment buffer (k-groups 4..7) included."""
    n = 1
    d, h, w = dims
    w3 = rnd((3, 3, 3, c, k2), 21, 0.2)
    w1 = (torch.arange(c * k2, dtype=torch.float32).reshape(1, 1, 1, c, k2) + 1.0) / 8.0      # distinct, exact in fp32
    dy = torch.zeros((n, d, h, w, k2))
    dy2 = torch.zeros((n, d, h, w, k2))
    want = torch.zeros((n, d, h, w, c))
    i = 0
    for tile_x in (0, 16):
        for (pz, py, px) in ((0, 0, 0), (2, 2, 14)):
            for oz in (0, 1):
                for oy in (0, 1):
                    for ox in (0, 1):
                        k = (3 + 5 * i + flip) % k2
                        i += 1
                        dy2[0, pz + oz, py + oy, tile_x + px + ox, k] = 1.0
                        want[0, pz + oz, py + oy, tile_x + px + ox, :] = w1[0, 0, 0, :, k]
    used = set(int(v) for v in dy2.sum(dim=(0, 1, 2, 3)).nonzero().flatten())
    assert set(k // 4 for k in used) == set(range(k2 // 4)), sorted(used)      # both halves of every k-group occur
    dx = torch.full((n, d, h, w, c), float('nan'), device=dev())
    run_pair(dy.to(dev()), w3, dy2.to(dev()), w1, dx, False, want=1)
    assert torch.equal(dx.cpu(), want), 'max difference %r' % float((dx.cpu() - want).abs().max())


def test_slab_views_and_their_neighbouring_bytes(monkeypatch):
    """dx written into a channel slice of a slab with 16 pad channels, dy2 read from a slab view with ld2 > K2: the result meets the
    oracle, the pad channels and the guard bands around every buffer keep their fill"""
    n, dims, k2, c = 2, (4, 8, 32), 24, 48
    q = case_data(n, dims, k2, c)
    g = install(monkeypatch, FILL)
    dxb, dxv = g.slab((n,) + dims + (c,), torch.float32, dev(), lead=8, tail=8)
    d2b, d2v = g.slab((n,) + dims + (k2,), torch.float32, dev(), lead=4, tail=4, values=q['dy2'])
    dyb, dyv = g.slab((n,) + dims + (k2,), torch.float32, dev(), lead=4, tail=0, values=q['dy'])
    run_pair(dyv, q['w3'], d2v, q['w1'], dxv, False, want=1)
    check(dxv, q['ref'], q['bound'], 'pair on slab views')
    dxv.copy_(q['old'].to(dev()))
    run_pair(dyv, q['w3'], d2v, q['w1'], dxv, True, want=1)
    check(dxv, q['ref'] + q['old'].double(), q['bound'] + q['old'].double().abs(), 'accumulating pair on slab views')
    assert g.untouched(dxb, 8, c) and g.untouched(d2b, 4, k2) and g.untouched(dyb, 4, k2)
    assert g.check() >= 3


def test_operands_the_form_cannot_read_take_two_launches():
    """dy2 four bytes off its 16-byte boundary, and K2 = 12 (no whole k-groups): two launches each, same result"""
    n, dims, k2, c = 1, (5, 6, 14), 24, 24
    q = case_data(n, dims, k2, c)
    flat = torch.empty(q['dy2'].numel() + 1, device=dev())
    dy2 = flat[1:].view(q['dy2'].shape)
    dy2.copy_(q['dy2'].to(dev()))
    assert dy2.data_ptr() % 16 == 4
    dx = torch.full((n,) + dims + (c,), float('nan'), device=dev())
    run_pair(q['dy'].to(dev()), q['w3'], dy2, q['w1'], dx, False, want=2)
    check(dx, q['ref'], q['bound'], 'pair with dy2 off its boundary')
    n, dims, k2, c = 1, (4, 4, 12), 12, 16
    q = case_data(n, dims, k2, c)
    dx = torch.full((n,) + dims + (c,), float('nan'), device=dev())
    run_pair(q['dy'].to(dev()), q['w3'], q['dy2'].to(dev()), q['w1'], dx, False, want=2)
    check(dx, q['ref'], q['bound'], 'pair with K2 = 12')


def test_two_runs_are_identical_and_both_forms_agree(monkeypatch):
    n, dims, k2, c = 1, (32, 32, 96), 64, 16
    q = case_data(n, dims, k2, c)
    dy, dy2 = q['dy'].to(dev()), q['dy2'].to(dev())
    out = []
    for _ in range(2):
        dx = torch.full((n,) + dims + (c,), float('nan'), device=dev())
        run_pair(dy, q['w3'], dy2, q['w1'], dx, False, want=1)
        out.append(dx.cpu())
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    monkeypatch.setenv('BTS_IGEMM_NOPAIR', '1')
    dx = torch.full((n,) + dims + (c,), float('nan'), device=dev())
    names = run_pair(dy, q['w3'], dy2, q['w1'], dx, False, want=2)
    assert names[0] == 'w3_kernel', names
    diff = (dx.cpu().double() - out[0].double()).abs()
    assert bool((diff <= 2 * tol_of(q['bound'])).all()), float((diff / tol_of(q['bound'])).max())
    print('one launch against two: worst |difference| %.3e, worst difference / bound %.4f' % (float(diff.max()), float((diff / tol_of(q['bound'])).max())))
