"""-m gpu: csrc/ensemble.hip (bts_ensemble_update, bts_uncertainty_finish, bts_uncertainty_confusion) against tests/ensemble_ref.py.

Shapes: a single element; flat counts below, at and one over a 16-byte group of four floats (and, for the levels, of the sixteen a lane
takes at once); odd extents; a whole number of groups and a ragged tail beyond it; C = 1, 3, 4 (every specialisation of the finish kernel and three of the table's); and views one float (one byte)
past a 16-byte boundary, the element-by-element path.

Welford.  The kernel rounds every operation on its own (the update is compiled with contraction into fused multiply-adds switched off,
and its division is the IEEE one), so it must give the float32 numpy recurrence BIT FOR BIT; that is what holds on the device -- with
the multiply and the add of m2 fused it did not, by one ulp -- and what is asserted.  Independently both are held to the
float64 two-pass moments within a bound from the rounding count per update.  With members in [0, 1] every intermediate but m2 lies in
[-1, 1], where a rounding errs by at most v = 2^-25.  Mean: the update mean_k = mean + (p - mean) / k rounds three times, r_k <=
v (1 + 2 / k), and damps the error it inherits by (1 - 1/k): e_k <= sum_j (j / k) r_j <= v ((k + 1) / 2 + 2).  m2: the increment
d (p - mean_k) sees e_(k-1) in d and e_k in the other factor, both of magnitude <= 1: <= v (k + 5); d, p - mean_k and their product round
once each: 3 v; the sum rounds to half an ulp of m2 <= k / 4: <= v k / 2.  Together v (1.5 k + 8) per update:
    mean_bound(M) = v ((M + 1) / 2 + 2)              3.1e-7 at M = 16, 1.5e-7 at the M = 5 used here
    m2_bound(M)   = v sum_{k=2..M} (1.5 k + 8)       9.6e-6 at M = 16, 1.6e-6 at M = 5
both under the 1e-5 allowed at M <= 16.  A wrong recurrence (k off by one, mean read after its update) misses by 1e-2.

Levels.  The device evaluates 100 h and 200 sigma in float32; against the float64 levels it may differ by one, and only where the exact
value lies within 1e-3 of a half-integer (the float32 evaluation moves 100 h by about 2e-5); at most 1 % of the voxels may lie in that band
(uniform random p: 0.2 %)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ensemble_ref as E  # noqa: E402
import guard_alloc  # noqa: E402

VOLUMES = [(1, 1, 1), (1, 1, 3), (1, 2, 2), (3, 5, 7), (16, 16, 16), (17, 16, 16)]
CHANNELS = [1, 3, 4]
V25 = 2.0 ** -25


def mean_bound(m):
    return V25 * ((m + 1) / 2.0 + 2.0)


def m2_bound(m):
    return V25 * sum(1.5 * k + 8.0 for k in range(2, m + 1))


def dev():
    return torch.device('cuda', 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def ops():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops


def run_members(o, members, with_m2, offset=0):
    """fold the members on the device -> (mean, m2 or None) as numpy; offset: every buffer is a view that many floats into a larger one"""
    n = members[0].size

    def buf():
        return torch.empty(n + offset, dtype=torch.float32, device=dev())[offset:]
    mean, m2 = buf(), (buf() if with_m2 else None)
    for k, p in enumerate(members, 1):
        pv = buf()
        pv.copy_(gpu(p.reshape(-1)))
        assert pv.data_ptr() % 16 == 4 * (offset % 4)
        got = o.ensemble_update(pv, mean, m2, k)
        assert got[0] is mean and got[1] is m2
    return mean.cpu().numpy(), (None if m2 is None else m2.cpu().numpy())


def test_bounds_are_within_what_is_allowed():
    assert mean_bound(16) <= 1e-5 and m2_bound(16) <= 1e-5 and m2_bound(5) < 2e-6


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('vol', VOLUMES)
def test_welford_is_the_float32_numpy_recurrence_bit_for_bit(vol, c):
    o = ops()
    for kind, members in E.member_sets(vol + (c,), 100 * vol[0] + c).items():
        flat = [m.reshape(-1) for m in members]
        ref_mean, ref_m2 = E.welford(flat, np.float32)
        x_mean, x_m2 = E.exact_moments(flat)
        mean, m2 = run_members(o, flat, True)
        e_mean, e_m2 = float(np.abs(mean - x_mean).max()), float(np.abs(m2 - x_m2).max())
        print('%s %s C=%d: |mean - fp64| %.2e (bound %.2e), |m2 - fp64| %.2e (bound %.2e)' %
              (kind, vol, c, e_mean, mean_bound(5), e_m2, m2_bound(5)))
        assert np.array_equal(mean.view(np.uint32), ref_mean.view(np.uint32)), kind
        assert np.array_equal(m2.view(np.uint32), ref_m2.view(np.uint32)), kind
        assert e_mean <= mean_bound(5) and e_m2 <= m2_bound(5), kind
        only_mean, none = run_members(o, flat, False)                    # entropy mode: the mean alone, the same bits
        assert none is None and np.array_equal(only_mean.view(np.uint32), ref_mean.view(np.uint32)), kind


@pytest.mark.parametrize('n', [1, 3, 4, 5, 3 * 5 * 7 * 3])
def test_welford_on_views_one_float_off_a_16_byte_boundary(n):
    o = ops()
    members = [m.reshape(-1) for m in E.member_sets((n,), n)['random']]
    ref_mean, ref_m2 = E.welford(members, np.float32)
    mean, m2 = run_members(o, members, True, offset=1)
    assert np.array_equal(mean.view(np.uint32), ref_mean.view(np.uint32)) and np.array_equal(m2.view(np.uint32), ref_m2.view(np.uint32))


def test_a_wrong_recurrence_would_miss_the_bound():
    """the check has teeth: the recurrence with k off by one leaves the bound by orders of magnitude"""
    members = [m.reshape(-1) for m in E.member_sets((3, 5, 7, 3), 1)['random']]
    x_mean, _ = E.exact_moments(members)
    mean = members[0].astype(np.float64)
    for k, p in enumerate(members[1:], 1):                               # (k should count from 2)
        mean = mean + (p - mean) / k
    assert np.abs(mean - x_mean).max() > 1e-2


@pytest.mark.parametrize('with_m2', [False, True])
def test_first_member_ignores_what_the_accumulators_held(with_m2, monkeypatch):
    """k == 1 on accumulators filled with NaN bytes (guard_alloc's POISON) and on zeroed ones: the same bits, no band touched"""
    o = ops()
    n = 17 * 16 * 16 * 3
    p = E.member_sets((n,), 9)['random'][0]
    out = []
    for fill in (guard_alloc.POISON, 0x00):
        with monkeypatch.context() as mp:
            g = guard_alloc.install(mp, fill)
            pv = gpu(p)
            mean = g.empty(n, dtype=torch.float32, device=dev())
            m2 = g.empty(n, dtype=torch.float32, device=dev()) if with_m2 else None
            if fill == guard_alloc.POISON:
                assert bool(torch.isnan(mean).all())
            o.ensemble_update(pv, mean, m2, 1)
            g.check()
            out.append((mean.cpu().numpy(), None if m2 is None else m2.cpu().numpy()))
    assert np.array_equal(out[0][0].view(np.uint32), p.view(np.uint32)) and np.array_equal(out[1][0].view(np.uint32), p.view(np.uint32))
    if with_m2:
        assert not out[0][1].any() and not out[1][1].any() and not np.signbit(out[0][1]).any()


def test_update_refuses_bad_arguments():
    o = ops()
    p = torch.zeros(8, device=dev())
    with pytest.raises(ValueError, match='counts the members from 1'):
        o.ensemble_update(p, torch.zeros(8, device=dev()), None, 0)
    with pytest.raises(ValueError, match='needs the mean'):
        o.ensemble_update(p, None, None, 2)
    with pytest.raises(ValueError):
        o.ensemble_update(p, torch.zeros(7, device=dev()), None, 1)
    with pytest.raises(RuntimeError, match='BTS_ERR_UNSUPPORTED'):
        o.ensemble_update(p, p, None, 2)
    mean, m2 = o.ensemble_update(p, None, None, 1)                       # the first member may have its mean allocated
    assert m2 is None and tuple(mean.shape) == (8,) and mean.data_ptr() != p.data_ptr()


# ---- levels ----------------------------------------------------------------------------------------------------------------------
def check_levels(got, scaled, mask, what):
    ref = E.levels(scaled, mask)
    band = E.near_half(scaled)
    diff = got.astype(np.int32) - ref.astype(np.int32)
    print('%s: %d of %d within 1e-3 of a half-integer, %d levels differ' % (what, int(band.sum()), band.size, int((diff != 0).sum())))
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert int(np.abs(diff).max()) <= 1, what
    assert not (diff != 0)[~band].any(), what
    assert not got[np.broadcast_to(np.asarray(mask).reshape(got.shape[:-1] + (1,)) == 0, got.shape)].any(), what
    return band


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('vol', VOLUMES)
def test_levels_match_the_float64_formulas(vol, c):
    o = ops()
    rng = np.random.default_rng(7 * vol[0] + c)
    sets = E.member_sets(vol + (c,), 50 * vol[0] + c)
    mask = (rng.random(vol + (1,)) > 0.3).astype(np.float32)
    mask.reshape(-1)[0] = 1.0
    in_band = total = 0
    for kind, members in sets.items():
        mean32, m2_32 = E.welford(members, np.float32)
        got = o.uncertainty_finish(gpu(mean32), gpu(mask), 'entropy').cpu().numpy()
        band = check_levels(got, E.entropy_scaled(mean32), mask, 'entropy %s %s C=%d' % (kind, vol, c))
        in_band, total = in_band + int(band.sum()), total + band.size
        got = o.uncertainty_finish(gpu(mean32), gpu(mask), 'std', spread=gpu(m2_32), scale=1.0 / 5).cpu().numpy()
        band = check_levels(got, E.std_scaled(m2_32, 1.0 / 5), mask, 'std %s %s C=%d' % (kind, vol, c))
        in_band, total = in_band + int(band.sum()), total + band.size
        var32 = (m2_32 * np.float32(0.2)).astype(np.float32)             # a variance with scale 1, as after the way back
        got = o.uncertainty_finish(gpu(mean32), gpu(mask), 'std', spread=gpu(var32), scale=1.0).cpu().numpy()
        check_levels(got, E.std_scaled(var32, 1.0), mask, 'variance %s %s C=%d' % (kind, vol, c))
    if total >= 1000:
        assert in_band <= 0.01 * total
    uni = rng.random(vol + (c,), dtype=np.float32)                        # a single uniform member: every level of the entropy occurs
    got = o.uncertainty_finish(gpu(uni), gpu(mask), 'entropy').cpu().numpy()
    band = check_levels(got, E.entropy_scaled(uni), mask, 'entropy uniform %s C=%d' % (vol, c))
    if band.size >= 1000:
        assert band.mean() <= 0.01


def test_levels_at_the_ends_of_the_range_and_off_alignment():
    o = ops()
    p = np.array([0.0, 1.0, 0.5, -1e-3, 1.0 + 1e-3, 0.25, 1e-30, 1.0 - 2.0 ** -24], dtype=np.float32).reshape(8, 1)
    ones = np.ones((8, 1), dtype=np.float32)
    got = o.uncertainty_finish(gpu(p), gpu(ones), 'entropy').cpu().numpy().reshape(-1)
    assert got.tolist() == [0, 0, 100, 0, 0, 81, 0, 0]                   # 100 h(0.25) = 81.13
    s = np.array([0.0, 0.25, 0.3, -1.0, 1e-6, 0.0625, 4.0, 0.01], dtype=np.float32).reshape(8, 1)
    got = o.uncertainty_finish(gpu(p), gpu(ones), 'std', spread=gpu(s)).cpu().numpy().reshape(-1)
    assert got.tolist() == [0, 100, 100, 0, 0, 50, 100, 20]              # 200 sqrt: 0, 100, 109.5 -> 100, 0, 0.2, 50, 400 -> 100, 20
    rng = np.random.default_rng(3)
    for n in (15, 16, 17, 33):                                           # below, at and over the 16 levels a lane takes at once
        mean = rng.random((n, 1), dtype=np.float32)
        mask = (rng.random((n, 1)) > 0.3).astype(np.float32)
        outbig = torch.full((n + 16,), 201, dtype=torch.uint8, device=dev())
        o.uncertainty_finish(gpu(mean), gpu(mask), 'entropy', out=outbig[:n].view(n, 1))
        assert bool((outbig[n:] == 201).all())
        check_levels(outbig[:n].view(n, 1).cpu().numpy(), E.entropy_scaled(mean), mask, 'n = %d' % n)
    # views one float / one byte off a 16-byte boundary, sentinel-filled output: every level written, nothing beyond
    for c in CHANNELS:
        nv = 3 * 5 * 7
        mean = rng.random((nv, c), dtype=np.float32)
        mask = (rng.random((nv, 1)) > 0.3).astype(np.float32)
        big = torch.empty(nv * c + 1, dtype=torch.float32, device=dev())
        big[1:].copy_(gpu(mean.reshape(-1)))
        outbig = torch.full((nv * c + 2,), 201, dtype=torch.uint8, device=dev())
        mv, ov = big[1:].view(nv, c), outbig[1:-1].view(nv, c)
        assert mv.data_ptr() % 16 == 4 and ov.data_ptr() % 4 == 1
        got = o.uncertainty_finish(mv, gpu(mask), 'entropy', out=ov)
        assert got is ov and int(outbig[0]) == 201 and int(outbig[-1]) == 201
        check_levels(ov.cpu().numpy(), E.entropy_scaled(mean), mask, 'offset view C=%d' % c)


def test_finish_refuses_bad_arguments():
    o = ops()
    mean, mask = torch.zeros((4, 3), device=dev()), torch.ones((4, 1), device=dev())
    with pytest.raises(ValueError, match='mode'):
        o.uncertainty_finish(mean, mask, 'variance')
    with pytest.raises(ValueError, match='needs the spread'):
        o.uncertainty_finish(mean, mask, 'std')
    with pytest.raises(ValueError):
        o.uncertainty_finish(mean, torch.ones((5, 1), device=dev()))
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        o.uncertainty_finish(mean, mask, 'std', spread=mean, scale=-1.0)


# ---- the table -------------------------------------------------------------------------------------------------------------------
def maps(n, c, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([0, 0, 0, 1, 2, 3, 4, 255], dtype=np.uint8)
    t, p = vals[rng.integers(0, 8, size=n)], vals[rng.integers(0, 8, size=n)]
    u = rng.integers(0, 101, size=(n, c)).astype(np.uint8)
    u[rng.random((n, c)) < 0.5] = 0                                      # most of a scan is certain
    u.reshape(-1)[::97] = 255                                            # beyond the range: counted as 100, and inside the table
    m = (rng.random(n) > 0.25).astype(np.uint8)
    return t, p, u, m


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('vol', VOLUMES + [(33, 64, 64)])
def test_table_is_exact(vol, c):
    """(33, 64, 64): 8448 chunks, more than one workgroup and more than one pass of a lane's registers"""
    o = ops()
    n = vol[0] * vol[1] * vol[2]
    t, p, u, m = maps(n, c, n + c)
    cms = E.class_masks('regions') if c == 3 else [1 << (1 + k % 3) for k in range(c)]
    tg, pg, ug, mg = gpu(t), gpu(p), gpu(u), gpu(m)
    for mask, mdev in ((None, None), (m, mg)):
        ref = E.table(t, p, u, cms, mask)
        got = o.uncertainty_confusion(tg, pg, ug, cms, mask=mdev)
        assert got.dtype == torch.int64 and tuple(got.shape) == (c, 101, 4)
        assert np.array_equal(got.cpu().numpy(), ref)
        assert int(ref.sum()) == c * (n if mask is None else int(m.sum()))
        again = o.uncertainty_confusion(tg, pg, ug, cms, mask=mdev)
        assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()            # a second run: the same bytes
        o.uncertainty_confusion(tg, pg, ug, cms, mask=mdev, table=again)               # two calls into one buffer: the sum
        assert np.array_equal(again.cpu().numpy(), 2 * ref)


def test_table_special_cases():
    o = ops()
    n, c = 3 * 5 * 7, 3
    cms = E.class_masks('regions')
    t, p, u, m = maps(n, c, 5)
    assert (t == 4).any() and (t == 255).any()
    folded = o.uncertainty_confusion(gpu(t), gpu(p), gpu(u), cms).cpu().numpy()
    assert np.array_equal(folded, E.table(np.minimum(t, 3), np.minimum(p, 3), u, cms))          # 4 and 255 are class 3
    for level in (0, 100):                                                                      # one hot row per channel
        flat = np.full((n, c), level, dtype=np.uint8)
        got = o.uncertainty_confusion(gpu(t), gpu(p), gpu(flat), cms).cpu().numpy()
        assert np.array_equal(got, E.table(t, p, flat, cms)) and int(got[:, level].sum()) == c * n
    hot = o.uncertainty_confusion(gpu(np.zeros(n, np.uint8)), gpu(np.zeros(n, np.uint8)), gpu(np.zeros((n, c), np.uint8)), cms).cpu().numpy()
    assert int(hot[0, 0, 0]) == n and int(hot.sum()) == c * n                                   # one hot CELL per channel
    bg = o.uncertainty_confusion(gpu(np.zeros(n, np.uint8)), gpu(p), gpu(u), cms).cpu().numpy()  # an all-background truth
    assert np.array_equal(bg, E.table(np.zeros(n, np.uint8), p, u, cms)) and not bg[:, :, 2:].any()
    # views one byte off a 16-byte boundary: byte loads
    big = [gpu(np.concatenate([np.zeros(1, np.uint8), a.reshape(-1)])) for a in (t, p, u, m)]
    tv, pv, uv, mv = (b[1:] for b in big)
    assert tv.data_ptr() % 16 == 1
    got = o.uncertainty_confusion(tv, pv, uv.view(n, c), cms, mask=mv).cpu().numpy()
    assert np.array_equal(got, E.table(t, p, u, cms, m))


def test_table_refuses_bad_arguments():
    o = ops()
    t = torch.zeros(16, dtype=torch.uint8, device=dev())
    u = torch.zeros((16, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(ValueError):
        o.uncertainty_confusion(t, t, u, [2, 4])                         # two masks for three channels
    with pytest.raises(ValueError, match='class masks'):
        o.uncertainty_confusion(t, t, u, [2, 4, 16])                     # bit 4 with K = 4
    with pytest.raises(RuntimeError, match='BTS_ERR_UNSUPPORTED'):
        o.uncertainty_confusion(t, t, torch.zeros((16, 5), dtype=torch.uint8, device=dev()), [2] * 5)
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        o.uncertainty_confusion(t, t, u, [2, 4, 8], n_classes=9)
